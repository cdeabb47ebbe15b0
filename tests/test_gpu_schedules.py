"""One small factored graph through every stream schedule of the loss call (cat_amd/csrc/crf_host.hip: utterance-minor, staged,
two streams, one stream) and through the schedule switches nothing else reaches: serial_chains, no_overlap, ctc_after, segments,
grad_par3, no_fin_fold, gd_stage_launches on the device.

The graph is the calibration graph of test_small_graphs_spread_rows (S = 513, the 1024-thread geometry); T = 300 because the stage
plan cuts stages from T >= 256 only; B = 5: ragged lengths, an odd batch for the two-utterance kernel, 10 den workgroups -- far
below the staged schedule's limit.  The fp64 oracle's answer is computed once; every row is one call under its switches, held to
it as test_small_graphs_spread_rows holds its call (TOL, rel_err per utterance), plus what the row says about the kernel and the
streams the call took."""
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import fst_io
from tests.util import make_batch, post_err, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
B, T, V = 5, 300, 72

# (id, switches, kernel: prefix of last_den_kernel() or None, contains: substring of it or None, streams: ("ge" | "eq", n) or None,
#  fallbacks: (denominator, numerator) counts of last_fallback_counts() or None)
ROWS = [
    ("default", {}, "crf_fac_pair_kernel<true", None, ("ge", 2), None),
    ("gd_stage_launches", dict(gd_stage_launches=1), "crf_fac_pair_kernel<true", None, ("ge", 2), None),
    ("segments", dict(segments=1), "crf_fac_pair_kernel<false", None, None, None),
    ("grad_par3", dict(grad_par3=1), None, None, ("eq", 3), None),
    ("aux_stream", dict(aux_stream=1), None, None, ("eq", 3), None),
    ("no_overlap_gate", dict(no_overlap=1, ctc_after=0), "crf_fac_pair_kernel<false", None, ("eq", 2), None),
    ("no_overlap_ctc_after", dict(no_overlap=1, ctc_after=1), None, None, ("eq", 2), None),
    ("no_overlap_resident", dict(no_overlap=1, no_factored=1), "crf_res_pair_kernel", None, None, None),
    ("no_overlap_pair2", dict(no_overlap=1, fac_pair2=1, fac_threads=768), "crf_fac_pair2_kernel<false", None, None, None),
    ("staged_pair2", dict(fac_pair2=1, fac_threads=768), "crf_fac_pair2_kernel<true", None, None, None),
    ("serial_chains", dict(serial_chains=1), None, None, ("eq", 1), None),
    ("serial_chains_generic_grad", dict(serial_chains=1, no_fast_grad=1), None, None, ("eq", 1), None),
    ("no_fin_fold", dict(no_fin_fold=1), None, None, None, None),
    ("robust_all", dict(robust=1), None, None, None, (B, B)),
    ("robust_never", dict(robust=0), None, None, None, (0, 0)),
    ("batch_persist", dict(force_batch=1, bat_persist=1), None, "persist", None, None),
    ("batch_frames", dict(force_batch=1, bat_persist=0), None, "frame", None, None),
    ("streaming", dict(no_resident=1, no_batch=1), "crf_den_pair_kernel<false>", None, None, None),
]


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The graph file, the batch and the oracle's answers (combined loss, den only, numerator only): computed once, never written to."""
    from cat_amd.den_lm import synth_den_lm
    p = os.path.join(str(tmp_path_factory.mktemp("schedules")), "small.fst")
    g = synth_den_lm(V, 256, 16, 0, path=p)
    logits, labels, lx, ly = make_batch(g, B, T, V, ragged=True)
    gref = fst_io.read_fst(p)
    c = dict(path=p, logits=logits, labels=labels, lx=lx, ly=ly, ref=oracle.ctc_crf(gref, logits, labels, lx, ly, lamb=0.1),
             den=oracle.den(gref, logits, lx), ctc=oracle.ctc(logits, labels, lx, ly))
    for a in (logits, c["ref"]["grad"], c["den"][0], c["ctc"][0]):
        a.setflags(write=False)
    return c


def run_row(crf, case, opts):
    """One CTC_CRF_LOSS call under `opts` on a graph created under them -> (loss, grad, den kernel, streams, side stream, fallback counts)."""
    with crf._C.debug_opts(**opts):
        ctx = crf.CRFContext(case["path"], 0)
        x = torch.tensor(case["logits"], device="cuda:0", requires_grad=True)
        loss = crf.CTC_CRF_LOSS(lamb=0.1)(x, torch.tensor(case["labels"], dtype=torch.int32), torch.tensor(case["lx"], dtype=torch.int32),
                                          torch.tensor(case["ly"], dtype=torch.int32))
        kernel, streams, side = crf._C.last_den_kernel(), crf._C.last_call_streams(), crf._C.last_side_stream()
        falls = crf._C.last_fallback_counts(torch.cuda.current_stream().cuda_stream)
        loss.backward()
        out = float(loss.item()), x.grad.cpu().numpy()
        del ctx
    return out + (kernel, streams, side, falls)


@pytest.mark.parametrize("name,opts,kernel,contains,streams,fallbacks", ROWS, ids=[r[0] for r in ROWS])
def test_schedule_row(crf, case, name, opts, kernel, contains, streams, fallbacks):
    loss, grad, got_kernel, got_streams, side, got_falls = run_row(crf, case, opts)
    ref = case["ref"]
    print(name, "loss", loss, "oracle", ref["loss"], "rel_err", [rel_err(grad[b], ref["grad"][b]) for b in range(B)],
          got_kernel, got_streams, side, got_falls)
    assert abs(loss - ref["loss"]) <= TOL * abs(ref["loss"]), name
    for b in range(B):
        assert rel_err(grad[b], ref["grad"][b]) <= TOL, (name, b)
    if kernel is not None:
        assert got_kernel.startswith(kernel), (name, got_kernel)
    if contains is not None:
        assert contains in got_kernel, (name, got_kernel)
    if streams is not None and side.startswith("none"):
        print(f"{name}: this context has no side stream ({side}): the call ran on one stream, its stream count is not asserted")
    elif streams is not None:
        assert got_streams >= streams[1] if streams[0] == "ge" else got_streams == streams[1], (name, got_streams, side)
    if fallbacks is not None:
        assert got_falls == fallbacks, (name, got_falls)


def test_numerator_only(crf, case):
    """WARP_CTC_LOSS: no graph, the one-stream schedule with the numerator's grad half alone."""
    x = torch.tensor(case["logits"], device="cuda:0", requires_grad=True)
    loss = crf.WARP_CTC_LOSS(size_average=False)(x, torch.tensor(case["labels"], dtype=torch.int32), torch.tensor(case["lx"], dtype=torch.int32),
                                                 torch.tensor(case["ly"], dtype=torch.int32))
    streams = crf._C.last_call_streams()
    loss.backward()
    gref, cref, valid = case["ctc"]
    assert list(valid) == [1] * B
    print("numerator only: loss", loss.item(), "oracle", -cref.sum(), "rel_err", rel_err(x.grad.cpu().numpy(), -gref))
    assert streams == 1
    assert abs(loss.item() + cref.sum()) <= TOL * abs(cref.sum())
    assert rel_err(x.grad.cpu().numpy(), -gref) <= TOL


def test_den_only(crf, case):
    """gpu_den: the denominator alone, the one-stream schedule with the den half of the grad pass alone."""
    ctx = crf.CRFContext(case["path"], 0)
    lg = torch.tensor(case["logits"], device="cuda:0")
    gd, ca, cb = torch.zeros_like(lg), torch.zeros(B, device="cuda:0"), torch.zeros(B, device="cuda:0")
    crf._C.gpu_den(lg, gd, torch.tensor(case["lx"]).cuda(), ca, cb)
    kernel, streams = crf._C.last_den_kernel(), crf._C.last_call_streams()
    del ctx
    den = case["den"]
    print("den only:", kernel, streams, "post_err", post_err(gd.cpu().numpy(), np.asarray(den[0])))
    assert kernel.startswith("crf_fac_pair_kernel<false") and streams == 1, (kernel, streams)
    assert np.allclose(ca.cpu().numpy(), np.asarray(den[1]).ravel(), rtol=TOL, atol=0)
    assert np.allclose(cb.cpu().numpy(), np.asarray(den[2]).ravel(), rtol=TOL, atol=0)
    assert post_err(gd.cpu().numpy(), np.asarray(den[0])) <= TOL
