"""Row epilogues of the factored denominator recursions: the backward vector's PLANAR numbering (z entries of row rid at rid and
R + rid in LDS; the BP rows in memory keep 2 rid + output) in every kernel that shares it -- one utterance per workgroup on 1024 and
768 threads, rows on several lanes, two CUs per recursion, two utterances per workgroup -- and the ds_write_addtid_b32 stores of the
1024-thread kernels (last template argument of crf_fac_pair_kernel; switch fac_addtid = 1 / 0 forces them on / off for any graph).

Every case: workspace poisoned, two back-to-back calls on different inputs, the fp64 oracle for the loss terms and the full gradient
(1e-4), forward logZ against backward logZ (3e-5), posterior rows summing to one (3e-4), zeros beyond lx -- the helpers and tolerances
of tests/test_gpu_metric_shape.py -- and an assertion on the instantiation that ran.  Where a graph runs with the new stores on and off,
loss, gradient and both logZ are compared BIT FOR BIT: the arithmetic is the same, so any difference is a numbering bug."""
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import fst_io
from tests.util import crf_env, make_batch, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
LAMB = 0.1


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf


_graphs = {}


def _graph(tmp_path_factory, V, H, fanout):
    """(graph, path, the oracle's copy), built once per module."""
    key = (V, H, fanout)
    if key not in _graphs:
        from cat_amd.den_lm import synth_den_lm
        p = os.path.join(str(tmp_path_factory.mktemp("denlm")), f"den_lm_v{V}_h{H}_d{fanout}.fst")
        g = synth_den_lm(V, H, fanout, 0, path=p)
        _graphs[key] = (g, p, fst_io.read_fst(p))
    return _graphs[key]


def _run(crf, path, batches, B, **switches):
    """Two poisoned back-to-back calls under the graph-time switches -> (outputs, numerator posteriors, kernel, graph statistics)."""
    core = crf._C
    with crf_env(**switches):
        ctx = crf.CRFContext(path, 0)
    st = core.graph_stats(core.graph_for(torch.device("cuda", 0)))
    core.set_debug_poison(True)
    try:
        outs, s = [], 1.0 / B
        for lg, lab, lx, ly in batches:                     # back to back, no synchronisation in between
            x = torch.tensor(lg, device="cuda:0")
            outs.append(core.loss_fwd_bwd(x, torch.tensor(lab), torch.tensor(lx), torch.tensor(ly), s, s * (1 + LAMB),
                                          core.graph_for(x.device), True))
        torch.cuda.synchronize()
        kern = core.last_den_kernel()
        gctc = []
        for lg, lab, lx, ly in batches:
            x = torch.tensor(lg, device="cuda:0")
            gctc.append(core.loss_fwd_bwd(x, torch.tensor(lab), torch.tensor(lx), torch.tensor(ly), 0.0, -1.0, None, True)[1])
        torch.cuda.synchronize()
    finally:
        core.set_debug_poison(False)
    outs = [(float(loss.item()), grad.cpu().numpy(), {k: ex[k].cpu().numpy() for k in ("costs_alpha", "costs_beta", "costs_ctc", "invalid")})
            for loss, grad, ex in outs]
    gctc = [g.cpu().numpy() for g in gctc]
    del ctx
    return outs, gctc, kern, st


def _refs(gref, batches, idx):
    """The fp64 oracle on the utterances `idx` of every batch: computed once per case, shared by its runs."""
    refs = []
    for lg, lab, lx, ly in batches:
        off = np.concatenate([[0], np.cumsum(ly)])
        labs = np.concatenate([lab[off[i]:off[i + 1]] for i in idx]).astype(np.int32)
        refs.append(oracle.ctc_crf(gref, lg[idx], labs, lx[idx], ly[idx], lamb=LAMB, size_average=False, threads=3))
    return refs


def _check(batches, outs, gctc, refs, idx, B):
    for (lg, lab, lx, ly), (loss, grad, ex), gc, ref in zip(batches, outs, gctc, refs):
        assert np.isfinite(loss)
        ca, cb, cc = (ex[k].astype(np.float64) for k in ("costs_alpha", "costs_beta", "costs_ctc"))
        assert int(ex["invalid"].sum()) == 0
        assert abs(loss - (ca - (1 + LAMB) * cc).sum() / B) <= 1e-5 * abs(loss)
        assert np.allclose(ca, cb, rtol=3e-5, atol=0), (ca, cb)
        gden = grad * B + (1 + LAMB) * gc
        assert gden.min() >= -2e-5
        for b in range(B):
            n = int(lx[b])
            assert np.allclose(gden[b, :n].sum(-1), 1.0, atol=3e-4), (b, gden[b, :n].sum(-1))
            assert np.all(grad[b, n:] == 0.0)
        g3 = grad[idx] * B
        for j, b in enumerate(idx):
            assert abs(ca[b] - ref["costs_den"][j]) <= TOL * abs(ref["costs_den"][j])
            assert abs(cc[b] - ref["costs_ctc"][j]) <= TOL * abs(ref["costs_ctc"][j])
            e = rel_err(g3[j], ref["grad"][j])
            print(f"utterance {b} (lx={int(lx[b])}): grad err vs fp64 oracle {e:.2e}")
            assert e <= TOL


def _same_bits(a, b):
    for (la, ga, ea), (lb, gb, eb) in zip(a, b):
        assert np.float64(la).tobytes() == np.float64(lb).tobytes(), (la, lb)
        assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
        for k in ("costs_alpha", "costs_beta", "costs_ctc"):
            assert ea[k].tobytes() == eb[k].tobytes(), k


def _short_batch(g, V, T, seed):
    """Three utterances of T, 2 and 1 frames (one label each for the short ones): the first frame's clearing of the start entries and
    the vector a recursion ends on after one or two frames."""
    from cat_amd.den_lm import random_labels_from_graph
    rng = np.random.default_rng(seed)
    lg, _, _, _ = make_batch(g, 3, T, V, seed=seed, ragged=False)
    lx = np.array([T, 2, 1], dtype=np.int32)
    ly = np.array([T // 6, 1, 1], dtype=np.int32)
    lab = np.concatenate([random_labels_from_graph(g, int(n), rng) for n in ly]).astype(np.int32)
    return lg, lab, lx, ly


# (vocabulary, histories, fan-out), B, T, switches of every run, what the kernel's name must start with / end with per run, fac_geom
CASES = {
    # one slice of 64 backward rows, two forward: the smallest factored graph
    "small_1024": ((12, 64, 6), 3, 12, [dict(CRF_FAC_ADDTID=1), dict(CRF_FAC_ADDTID=0)],
                   [("crf_fac_pair_kernel<true,1024,", ",false,true,true>"), ("crf_fac_pair_kernel<true,1024,", ",false,true,false>")], 4),
    "small_768": ((12, 64, 6), 3, 12, [dict(CRF_FAC_THREADS=768)], [("crf_fac_pair_kernel<true,768,", ">")], None),
    # rows longer than a lane's 60 arcs (ML instantiation: the DPP butterfly in front of the epilogue).  synth_den_lm needs
    # histories >= vocabulary - 1, so the smallest graph with 64 tokens per history at V = 72 has H = 71 (S = 143): the planner keeps it on
    # the 1024-thread geometry, 4 743 of its 4 746 forward arcs in multi-lane rows
    "long_rows": ((72, 71, 64), 2, 10, [dict(CRF_FAC_ADDTID=1), dict(CRF_FAC_ADDTID=0)],
                  [("crf_fac_pair_kernel<true,1024,", ",true,true,true>"), ("crf_fac_pair_kernel<true,1024,", ",true,true,false>")], 4),
    # 33 slices per direction on 16 waves, the second copy of the gathered entries, the planner's own choice beside both forced ones
    "bench_graph": ((72, 2048, 24), 3, 12, [dict(CRF_FAC_ADDTID=1), dict(CRF_FAC_ADDTID=0), dict()],
                    [("crf_fac_pair_kernel<true,1024,", ",false,true,true>"), ("crf_fac_pair_kernel<true,1024,", ",false,true,false>"),
                     ("crf_fac_pair_kernel<true,1024,", ",false,true,true>")], 4),
    # two CUs per recursion: the peer's two planes cross every frame (and once more, in full, after the last)
    "two_cus": ((72, 3072, 24), 2, 24, [dict()], [("crf_fac2_pair_kernel<", ">")], 3),
    # two utterances per workgroup on the graph's second (512-thread) layout
    "two_utterances": ((72, 2048, 24), 144, 16, [dict()], [("crf_fac_pair2_kernel<true", ">")], 4),
}


@pytest.mark.parametrize("case", list(CASES))
def test_planar_backward_vector_and_addtid_stores(crf, tmp_path_factory, case):
    (V, H, fanout), B, T, runs, names, geom = CASES[case]
    g, p, gref = _graph(tmp_path_factory, V, H, fanout)
    batches = [make_batch(g, B, T, V, seed=0, ragged=True), make_batch(g, B, T, V, seed=7, ragged=False)]
    idx = np.arange(B) if B <= 4 else np.array([0, B // 2 - 1, B - 1])
    refs = _refs(gref, batches, idx)
    results = []
    for sw, (head, tail) in zip(runs, names):
        outs, gctc, kern, st = _run(crf, p, batches, B, **sw)
        assert st["fac"] == 1 and (geom is None or st["fac_geom"] == geom), st
        assert kern.startswith(head) and kern.endswith(tail), (sw, kern)
        _check(batches, outs, gctc, refs, idx, B)
        results.append(outs)
    for other in results[1:]:
        _same_bits(results[0], other)


@pytest.mark.parametrize("addtid", [1, 0])
def test_one_and_two_frame_utterances(crf, tmp_path_factory, addtid):
    """lx = 2 and lx = 1 beside a longer utterance on the small graph: the vector a backward recursion starts from (z_lab / z_end by
    planar entry), the rows of its only frames, the start entries cleared behind frame 0."""
    V = 12
    g, p, gref = _graph(tmp_path_factory, V, 64, 6)
    batches = [_short_batch(g, V, 12, 3), _short_batch(g, V, 12, 5)]
    idx = np.arange(3)
    outs, gctc, kern, st = _run(crf, p, batches, 3, CRF_FAC_ADDTID=addtid)
    assert st["fac"] == 1 and st["fac_geom"] == 4, st
    assert kern.startswith("crf_fac_pair_kernel<true,1024,") and kern.endswith(",true>" if addtid else ",false>"), kern
    _check(batches, outs, gctc, _refs(gref, batches, idx), idx, 3)
