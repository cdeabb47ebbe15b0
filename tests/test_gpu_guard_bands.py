"""GPU tests: every kernel family on buffers carved from one 0xFF-filled arena (tests/guard.py) -- 64 KiB of guard bytes on each side of
every device buffer of the call, a workspace of exactly crf_workspace_bytes, and (switch ws_gap) 256 untouched bytes behind every section
of it.  Every case runs the C ABI once, asserts that no guard byte and no byte between two sections changed, holds the results to the fp64
oracle as the parity tests do (TOL, rel_err per utterance, loss relative, rows t >= lx[b] exactly zero; alignments: tests/align_ref.py)
and asserts which kernel ran the denominator.  No case writes out of bounds on purpose: the checker's negative control is a CPU test
(tests/test_ws_sections.py)."""
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import fst_io
from cat_amd.den_lm import random_labels_from_graph, synth_den_lm
from tests import align_ref, guard
from tests.test_gpu_ctc_align import bound
from tests.test_gpu_ctc_align_logits import lse64, tolerance
from tests.test_gpu_ctc_logits import check as check_ctc_logits, reference as ctc_logits_reference, softmax64
from tests.test_gpu_parity import MODES, _mode
from tests.test_gpu_schedules import ROWS
from tests.util import log_softmax_np, make_batch, oracle_blank, rel_err, small_synth

pytestmark = pytest.mark.gpu
TOL = 1e-4
LAMB = 0.1
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DEV = torch.device("cuda", 0)

# what last_den_kernel() must say in each parity mode on the small T o LM graphs of the cases A, E and H (B = 5: groups of 8 utterances):
# (prefix, substring or None)
FAMILY = {
    "factored": ("crf_fac_pair_kernel<", ",1024,"), "factored_768": ("crf_fac_pair_kernel<", ",768,21,"),
    "factored_rcl": ("crf_fac_pair_kernel<", ",768,20,"), "factored_k2": ("crf_fac2_pair_kernel<768,", None),
    "factored_k2_1024": ("crf_fac2_pair_kernel<1024,", None), "factored_pair2": ("crf_fac_pair2_kernel<", ",768,"),
    "factored_pair2_512": ("crf_fac_pair2_kernel<", ",512,30,"), "resident": ("crf_res_pair_kernel", None),
    "streaming": ("crf_den_pair_kernel<false>", None), "batch": ("crf_batch_persist_kernel<8,4,true>", None),
    "batch_frames": ("crf_batch_frame_kernel<8,4,true>", None),
}


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf


def frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, dict):
            frozen(a)
    return d


def batch_for(g, V, T, lx, seed):
    """log-probs [B,T,V], labels that walk the graph (ly = lx // 6: a one-frame utterance has none), lx, ly."""
    rng = np.random.default_rng(seed)
    lx = np.asarray(lx, dtype=np.int32)
    logits = log_softmax_np(rng.normal(0.0, 1.0, size=(len(lx), T, V)) * 2.0)
    ly = (lx // 6).astype(np.int32)
    labels = np.concatenate([random_labels_from_graph(g, int(n), rng) for n in ly]).astype(np.int32)
    return logits, labels, lx, ly


def hold(out, ref, lx, what, costs=True):
    """Loss relative, rel_err per utterance, rows t >= lx[b] exactly zero -- as tests/test_gpu_parity.py and tests/test_gpu_schedules.py."""
    B = len(lx)
    grad = out["grad"]
    errs = [rel_err(grad[b], ref["grad"][b]) for b in range(B)]
    print(what, out["kernel"], "streams", out["streams"], "loss", out["loss"], "oracle", ref["loss"], "rel_err", errs)
    assert not np.isnan(grad).any(), (what, "a gradient row was not written")
    assert abs(out["loss"] - ref["loss"]) <= TOL * abs(ref["loss"]), (what, out["loss"], ref["loss"])
    for b in range(B):
        assert errs[b] <= TOL, (what, b, errs[b])
        assert np.all(grad[b, int(lx[b]):] == 0.0), (what, b, "rows past lx")
    if costs and out["costs_den"] is not None:
        for name, want in (("costs_den", ref["costs_den"]), ("costs_beta", ref["costs_den"]), ("costs_ctc", ref["costs_ctc"])):
            assert np.all(np.abs(out[name] - want) <= TOL * np.maximum(1.0, np.abs(want))), (what, name, out[name], want)
        assert np.all(out["invalid"] == 0), (what, out["invalid"])


def family(kernel, mode, what):
    prefix, sub = FAMILY[mode]
    assert kernel.startswith(prefix) and (sub is None or sub in kernel), (what, mode, kernel)


def loss_call(crf, path, case, switches, fused_x=None, null_outputs=False, mode=None):
    """One crf_loss_fwd_bwd (fused_x: crf_loss_fwd_bwd_logits on that raw input) on a graph created under the switches, on carved buffers."""
    core = crf._C
    B = len(case["lx"])
    cm = _mode(mode) if mode else core.debug_opts()
    with cm, core.debug_opts(**switches):
        ctx = crf.CRFContext(path, 0)
        x = fused_x if fused_x is not None else torch.tensor(case["logits"])
        out = guard.run_loss(core, core.graph_for(DEV), x, case["labels"], case["lx"], case["ly"], 1.0 / B, (1.0 + LAMB) / B,
                             fused=fused_x is not None, null_outputs=null_outputs)
        out["side"] = core.last_side_stream()
        del ctx
    return out


def gap_opts(gap):
    return dict(ws_gap=gap) if gap else {}


# ---------------------------------------------------------------------------------------------------------------------------------
# A, E, H: the small T o LM graph with V % 4 != 0, an odd batch, T % 16 != 0, lx = T, block edges and one frame, one empty transcript
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(tmp_path_factory):
    g, p = small_synth(tmp_path_factory.mktemp("guard_small"), 13, 40, 6, 5)
    logits, labels, lx, ly = batch_for(g, 13, 37, (37, 36, 17, 1, 16), seed=3)
    assert ly.tolist() == [6, 6, 2, 0, 2]
    gref = fst_io.read_fst(p)
    case = dict(path=p, logits=logits, labels=labels, lx=lx, ly=ly, ref=oracle.ctc_crf(gref, logits, labels, lx, ly, lamb=LAMB),
                ctc=oracle.ctc(logits, labels, lx, ly))
    # the fused log_softmax: raw values rounded to each dtype, the oracle on log_softmax of the upcast values, and its gradient taken
    # through log_softmax in fp64: d/dx = G - softmax(x) * sum_v G
    raw = torch.tensor(np.random.default_rng(5).normal(size=(5, 37, 13)) * 3.0, dtype=torch.float32)
    case["fused"] = {}
    for name, dt in DTYPES.items():
        xr = raw.to(dt)
        xh = xr.float().numpy().astype(np.float64)
        r = oracle.ctc_crf(gref, log_softmax_np(xh), labels, lx, ly, lamb=LAMB)
        G = r["grad"].astype(np.float64)
        r["grad"] = G - softmax64(xh) * G.sum(-1, keepdims=True)
        case["fused"][name] = (xr, frozen(r))
    return frozen(case)


@pytest.mark.parametrize("gap", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_families(crf, small, mode, gap):
    """Case A."""
    out = loss_call(crf, small["path"], small, gap_opts(gap), mode=mode)
    family(out["kernel"], mode, "A")
    hold(out, small["ref"], small["lx"], ("A", mode, gap))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("mode", ["factored", "resident", "batch"])
def test_fused_loss(crf, small, mode, dtype):
    """Case E: crf_loss_fwd_bwd_logits; the 16-bit inputs start 2 bytes past a multiple of 256."""
    xr, ref = small["fused"][dtype]
    core = crf._C
    with _mode(mode), core.debug_opts(ws_gap=1):
        ctx = crf.CRFContext(small["path"], 0)
        out = guard.run_loss(core, core.graph_for(DEV), xr, small["labels"], small["lx"], small["ly"], 0.2, 0.2 * (1.0 + LAMB), fused=True,
                             misalign=0 if dtype == "fp32" else 2)
        del ctx
    family(out["kernel"], mode, "E")
    hold(out, ref, small["lx"], ("E", mode, dtype))
    assert float(np.abs(out["grad"].sum(-1)).max()) <= 1e-5      # (every frame's gradient sums to zero: test_fused_log_softmax's bound)


@pytest.mark.parametrize("mode", ["factored", "batch", "streaming", "numerator"])
def test_null_optional_outputs(crf, small, mode):
    """Case H: costs_den_dev, costs_beta_dev, costs_ctc_dev and invalid_dev all NULL (every store through them sits behind a test of the
    pointer in finalize_body, cat_amd/csrc/k_robust.hip; nothing else writes through them)."""
    core = crf._C
    if mode == "numerator":
        with core.debug_opts(ws_gap=1):
            out = guard.run_loss(core, None, torch.tensor(small["logits"]), small["labels"], small["lx"], small["ly"], 0.0, -1.0, null_outputs=True)
        gref, cref, valid = small["ctc"]
        hold(out, dict(loss=float(cref.sum()), grad=gref), small["lx"], ("H", mode))
    else:
        out = loss_call(crf, small["path"], small, dict(ws_gap=1), null_outputs=True, mode=mode)
        family(out["kernel"], mode, "H")
        hold(out, small["ref"], small["lx"], ("H", mode))
    assert out["costs_den"] is None and out["invalid"] is None


# ---------------------------------------------------------------------------------------------------------------------------------
# I: a graph WITHOUT the T o LM structure -- rows of 300 arcs (sub-rows, virtual copies of their entries), states entered with several
# labels: most rows of the utterance-minor kernels take the per-row path beside the arc streams
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hub(tmp_path_factory):
    from tests import general_graphs as gg
    p, g, V = gg.catalogue("hub", tmp_path_factory.mktemp("guard_hub"))
    logits, labels, lx, ly = gg.batch(V, 2.0, seed=41)
    return frozen(dict(path=p, logits=logits, labels=labels, lx=lx, ly=ly, ref=oracle.ctc_crf(g, logits, labels, lx, ly, lamb=LAMB)))


@pytest.mark.parametrize("gap", [0, 1])
@pytest.mark.parametrize("mode", ["resident", "batch", "streaming"])
def test_general_graph_families(crf, hub, mode, gap):
    """Case I: tests/general_graphs.py's `hub` (S = 400, one state entered by 300 arcs of one class and left by 300 arcs), B = 4 with
    utterances of two frames and of one."""
    out = loss_call(crf, hub["path"], hub, gap_opts(gap), mode=mode)
    want = {"resident": "crf_res_pair_kernel", "batch": "crf_batch_persist_kernel<8,4,", "streaming": "crf_den_pair_kernel<false>"}[mode]
    assert out["kernel"].startswith(want), (mode, out["kernel"])
    hold(out, hub["ref"], hub["lx"], ("I", mode, gap))


# ---------------------------------------------------------------------------------------------------------------------------------
# B: every schedule row on the S = 513 graph, with 16-frame blocks that do not divide T and utterances around the staging threshold
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sched(tmp_path_factory):
    p = os.path.join(str(tmp_path_factory.mktemp("guard_sched")), "small.fst")
    g = synth_den_lm(72, 256, 16, 0, path=p)
    logits, labels, lx, ly = batch_for(g, 72, 301, (301, 300, 257, 255, 17), seed=0)
    return frozen(dict(path=p, logits=logits, labels=labels, lx=lx, ly=ly,
                       ref=oracle.ctc_crf(fst_io.read_fst(p), logits, labels, lx, ly, lamb=LAMB)))


@pytest.mark.parametrize("name,opts,kernel,contains,streams,fallbacks", ROWS, ids=[r[0] for r in ROWS])
def test_schedule_rows(crf, sched, name, opts, kernel, contains, streams, fallbacks):
    """Case B: tests/test_gpu_schedules.py's rows with ws_gap = 1, T = 301 and lx = (301, 300, 257, 255, 17), each with its kernel, stream and
    fallback assertions."""
    out = loss_call(crf, sched["path"], sched, dict(opts, ws_gap=1))
    hold(out, sched["ref"], sched["lx"], ("B", name))
    got_kernel, got_streams, side = out["kernel"], out["streams"], out["side"]
    if kernel is not None:
        assert got_kernel.startswith(kernel), (name, got_kernel)
    if contains is not None:
        assert contains in got_kernel, (name, got_kernel)
    if streams is not None and side.startswith("none"):
        print(f"{name}: this context has no side stream ({side}): the call ran on one stream, its stream count is not asserted")
    elif streams is not None:
        assert got_streams >= streams[1] if streams[0] == "ge" else got_streams == streams[1], (name, got_streams, side)
    if fallbacks is not None:
        assert out["fallbacks"] == fallbacks, (name, out["fallbacks"])


# ---------------------------------------------------------------------------------------------------------------------------------
# C: utterance-minor kernels with seven padding utterances
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def groups(tmp_path_factory):
    g, p = small_synth(tmp_path_factory.mktemp("guard_groups"), 12, 40, 6, 5)
    logits, labels, lx, ly = make_batch(g, 9, 31, 12, seed=9, ragged=True)
    return frozen(dict(path=p, logits=logits, labels=labels, lx=lx, ly=ly,
                       ref=oracle.ctc_crf(fst_io.read_fst(p), logits, labels, lx, ly, lamb=LAMB)))


@pytest.mark.parametrize("no_fac", [0, 1])
@pytest.mark.parametrize("persist", [0, 1])
def test_utterance_minor_padding(crf, groups, persist, no_fac):
    """Case C: B = 9 in groups of 8: Bp = 16."""
    out = loss_call(crf, groups["path"], groups, dict(force_batch=1, bat_persist=persist, bat_ul=8, bat_no_fac=no_fac, ws_gap=1))
    assert out["kernel"] == f"crf_batch_{'persist' if persist else 'frame'}_kernel<8,4,{'false' if no_fac else 'true'}>", out["kernel"]
    hold(out, groups["ref"], groups["lx"], ("C", persist, no_fac))


# ---------------------------------------------------------------------------------------------------------------------------------
# D: state vectors in global memory
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(tmp_path_factory):
    p = os.path.join(str(tmp_path_factory.mktemp("guard_big")), "big.fst")
    g = synth_den_lm(72, 10000, 8, seed=3, path=p)
    logits, labels, lx, ly = make_batch(g, 2, 40, 72, seed=9, ragged=True)
    return frozen(dict(path=p, logits=logits, labels=labels, lx=lx, ly=ly,
                       ref=oracle.ctc_crf(fst_io.read_fst(p), logits, labels, lx, ly, lamb=LAMB)))


@pytest.mark.parametrize("robust", [None, 1])
@pytest.mark.parametrize("path", ["batch", "streaming"])
def test_global_memory_vectors(crf, big, path, robust):
    """Case D: the S = 20 001 graph of test_large_graph_global_vectors on both of its paths; robust = 1: every utterance once more through the
    log-domain fallback, whose fp64 vectors live in the workspace's gvec section for a graph of this size."""
    opts = dict(ws_gap=1, no_batch=1 if path == "streaming" else 0)
    if robust is not None:
        opts["robust"] = robust
    out = loss_call(crf, big["path"], big, opts)
    assert dict((n, b) for n, _, b in out["sections"])["gvec"] > 0
    assert out["kernel"].startswith("crf_batch_" if path == "batch" else "crf_den_pair_kernel<true>"), out["kernel"]
    if robust:
        assert out["fallbacks"] == (2, 2), out["fallbacks"]
    hold(out, big["ref"], big["lx"], ("D", path, robust))


# ---------------------------------------------------------------------------------------------------------------------------------
# F: numerator only, every crf_ctc_pair_kernel<NI>, both layouts, any blank, 16-bit rows on odd element indices
# ---------------------------------------------------------------------------------------------------------------------------------
V_CTC = 37
_CTC = {}


def ctc_case(L, blank):
    """Three utterances, the longest with L labels over T = 2 L + 60 frames (tests/test_gpu_ctc_logits.py::make_batch's lengths): raw values
    per dtype with the oracle's answer on log_softmax of the upcast values, and the fp32 log-probs with the oracle's answer on them."""
    key = (L, blank)
    if key not in _CTC:
        _CTC.clear()
        rng = np.random.default_rng(1000 + L + 7 * blank)
        T = 2 * L + 60
        lx = np.array([T, T // 3, T // 5], dtype=np.int32)
        ly = np.array([L, max(1, min(40, L // 8)), min(7, L)], dtype=np.int32)
        pool = np.array([v for v in range(V_CTC) if v != blank])
        lab = [pool[rng.integers(0, len(pool), size=int(ly[0]))],
               np.repeat(pool[rng.integers(0, len(pool), size=(int(ly[1]) + 2) // 3)], 3)[:int(ly[1])],
               pool[rng.integers(0, len(pool), size=int(ly[2]))]]
        labels = np.concatenate(lab).astype(np.int32)
        raw = torch.tensor(rng.normal(0.0, 2.0, size=(3, T, V_CTC)), dtype=torch.float32)
        c = dict(labels=labels, lx=lx, ly=ly, raw={})
        for name, dt in DTYPES.items():
            xr = raw.to(dt)
            _, ref, c64, valid = ctc_logits_reference(xr, labels, lx, ly, blank)
            assert valid.all() and np.isfinite(c64).all()
            c["raw"][name] = (xr, ref, c64)
        logp = log_softmax_np(raw.numpy().astype(np.float64))
        g64, c64, valid = oracle_blank(logp, labels, lx, ly, blank)
        assert valid.all()
        c["logp"] = (torch.tensor(logp), g64, c64)
        _CTC[key] = frozen(c)
    return _CTC[key]


@pytest.mark.parametrize("blank", [0, V_CTC - 1, 11])
@pytest.mark.parametrize("L", [255, 511, 1023, 1024])
def test_numerator_only(crf, L, blank):
    """Case F: crf_ctc_fwd_bwd and crf_ctc_fwd_bwd_logits (fp32, bf16, fp16), batch-major and time-major, default chains and robust_ctc = 1.
    2 L + 1 = 511, 1023, 2047, 2049 states: one, two, four and five states per thread of crf_ctc_pair_kernel.  The 16-bit inputs start 2
    bytes past a multiple of 256, and V * B = 111 is odd: time-major rows start on odd element indices (crf_ctc_fwd_bwd_logits reads its
    input element by element, ld_x in cat_amd/csrc/crf_device.h: 2-byte alignment is all it needs, as include/ctc_crf_hip.h says)."""
    core = crf._C
    c = ctc_case(L, blank)
    labels, lx, ly = c["labels"], c["lx"], c["ly"]
    for robust in (0, 1):
        with core.debug_opts(ws_gap=1, **(dict(robust_ctc=1) if robust else {})):
            for tm in (False, True):
                for kind in ("logp", "fp32", "bf16", "fp16"):
                    x, ref, c64 = c["logp"] if kind == "logp" else c["raw"][kind]
                    xx = x.transpose(0, 1).contiguous() if tm else x
                    out = guard.run_loss(core, None, xx, labels, lx, ly, 0.0, -1.0, fused=kind != "logp", time_major=tm, blank=blank,
                                         misalign=2 if kind in ("bf16", "fp16") else 0)
                    g = np.ascontiguousarray(out["grad"].transpose(1, 0, 2)) if tm else out["grad"]
                    what = ("F", L, blank, kind, "time-major" if tm else "batch-major", "robust_ctc" if robust else "default")
                    if robust:
                        assert out["fallbacks"] == (0, 3), (what, out["fallbacks"])
                    assert np.all(out["invalid"] == 0), what
                    assert abs(out["loss"] - c64.sum()) <= TOL * abs(c64.sum()), (what, out["loss"], c64.sum())
                    if kind == "logp":
                        assert not np.isnan(g).any(), what
                        for b in range(3):
                            err = rel_err(g[b], ref[b])
                            print(what, "utterance", b, "cost", out["costs_ctc"][b], c64[b], "grad rel_err", err)
                            assert abs(out["costs_ctc"][b] - c64[b]) <= TOL * max(1.0, abs(c64[b])), (what, b)
                            assert err <= TOL, (what, b, err)
                            assert np.all(g[b, int(lx[b]):] == 0.0), (what, b)
                    else:
                        check_ctc_logits(out["costs_ctc"].astype(np.float64), g, ref, c64, lx, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# G: forced alignment
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [0, 31, 32])
@pytest.mark.parametrize("V", [37, 257])
def test_alignment(crf, V, L):
    """Case G: crf_ctc_align and crf_ctc_align_logits (fp32, bf16, fp16), both layouts; V = 37 / 257: 16 / 64 lanes per frame in
    crf_align_lse_kernel; B * T = 105 frames: the last workgroup of either lse kernel is partly empty; 2 L + 1 = 1, 63, 65 states: 64 and
    128 back-pointer columns.  Utterance 0: L labels over all 35 frames; 1: no frames (invalid); 2: a frame of -inf (dead)."""
    core = crf._C
    B, T, blank = 3, 35, V // 3
    rng = np.random.default_rng(50 * V + L)
    pool = np.array([v for v in range(V) if v != blank])
    lab0 = pool[rng.permutation(len(pool))[:L]]                       # (no repeats: L <= 32 labels fit 35 frames)
    labs = [lab0, pool[rng.integers(0, len(pool), size=L // 2)], pool[rng.integers(0, len(pool), size=min(L, 10))]]
    lx, ly = np.array([T, 0, T - 1]), np.array([len(a) for a in labs])
    labels = np.concatenate(labs).astype(np.int32)
    raw = rng.normal(0.0, 2.0, size=(B, T, V)).astype(np.float32)
    raw[2, 11, :] = -np.inf
    res = {}
    for kind in ("logp", "fp32", "bf16", "fp16"):
        if kind == "logp":
            with np.errstate(invalid="ignore"):
                x = torch.tensor(raw).log_softmax(-1)
            x[2, 11, :] = -np.inf
        else:
            x = torch.tensor(raw).to(DTYPES[kind])
        xh = x.float().numpy()
        for tm in (False, True):
            with core.debug_opts(ws_gap=1):
                pos, sc, inv = guard.run_align(core, x.transpose(0, 1).contiguous() if tm else x, labels, lx, ly, blank, fused=kind != "logp",
                                               time_major=tm, misalign=2 if kind in ("bf16", "fp16") else 0)
            what = ("G", V, L, kind, tm)
            assert inv.tolist() == [0, 1, 0], (what, inv)
            for b in (1, 2):
                assert sc[b] == -np.inf and np.all(pos[b] == -2), (what, b)
            align_ref.check_path(pos[0], lab0, T, blank)
            if kind == "logp":
                ref, rpos = align_ref.viterbi(xh[0], lab0, blank)
                mine = align_ref.path_score(xh[0], pos[0], lab0, T, blank)
                tol = bound(T, ref)
            else:
                lse = lse64(xh[0])
                lsm = xh[0].astype(np.float64) - lse[:, None]
                ref, rpos = align_ref.viterbi(lsm, lab0, blank)
                mine = align_ref.path_score(lsm, pos[0], lab0, T, blank)
                tol = tolerance(T, V, align_ref.path_score(xh[0], pos[0], lab0, T, blank), lse)
            print(what, "score", sc[0], "ref", ref, "returned path", mine, "tol", tol)
            assert rpos is not None and abs(sc[0] - ref) <= tol and abs(mine - ref) <= tol, (what, sc[0], mine, ref, tol)
            res[(kind, tm)] = (pos, sc)
        assert np.array_equal(res[(kind, False)][0], res[(kind, True)][0])                       # the layouts agree bit for bit
        assert np.array_equal(res[(kind, False)][1].view(np.int32), res[(kind, True)][1].view(np.int32))
