"""GPU tests: every denominator kernel family on graphs WITHOUT the T o LM structure -- states entered with several labels, rows of
300 arcs cut into sub-rows, dead ends, unreachable states, thousands of rows, parallel arcs, one final state -- and on T o LM graphs
with three arcs changed (tests/general_graphs.py; the host-side checks of the same graphs: tests/test_general_graph_layouts.py), against
the fp64 oracle.  Before this file the only graphs without the structure that reached a GPU had at most five states.

Batches: B = 4, T = 40, lx = (40, 23, 2, 1) -- for the `default` family once more with lx[3] = 0 -- log_softmax(normal * sigma) with
sigma = 2 (and 8 for `hub` and `one_final`), random labels with ly <= lx // 3, lamb = 0.1, both size_average values across the
catalogue.  Every case holds, with the project's tolerance and metrics (TOL = 1e-4; tests/util.py rel_err with the fuzz's floor,
post_err): loss and per-utterance gradient of CTC_CRF_LOSS; gamma_den entry-wise and both log Z values of `gpu_den` (the den-only call);
frames at or past lx exactly zero; classes no arc carries exactly zero; no NaN / inf; and which kernel ran.  Each case prints one ROW
line (profiles/general_graph_families.txt is made of them)."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from tests import general_graphs as gg
from tests.test_gpu_parity import MODES, TOL, _mode
from tests.util import crf_env, post_err, rel_err

pytestmark = pytest.mark.gpu
LAMB = 0.1
DEV = torch.device("cuda", 0)
B = len(gg.LX)

# family -> (mode of tests/test_gpu_parity.py or None, further switches, res_K forced or None, what last_den_kernel() must say)
FAMILIES = {
    "default": (None, {}, None, lambda k: len(k) > 0),
    "resident_k1": ("resident", dict(CRF_RES_MINK=1), 1, lambda k: k.startswith("crf_res_pair_kernel")),
    "resident_k2": ("resident", dict(CRF_RES_MINK=2), 2, lambda k: k.startswith("crf_res_pair_kernel")),
    "resident_k4": ("resident", dict(CRF_RES_MINK=4), 4, lambda k: k.startswith("crf_res_pair_kernel")),
    "streaming": ("streaming", {}, None, lambda k: k.startswith("crf_den_pair_kernel")),
    "batch_ul8": ("batch", dict(CRF_BAT_UL=8), None, lambda k: "persist" in k),
    "batch_ul64": ("batch", dict(CRF_BAT_UL=64), None, lambda k: "persist" in k),
    "batch_frames_ul16": ("batch_frames", dict(CRF_BAT_UL=16), None, lambda k: "frame" in k),
}
# (`lds_edge` with K = 1 is left out: crf_den_kernels says such a call does not take the generic register-resident kernels -- the rows
# do not fit the LDS beside V = 72 classes -- which tests/test_general_graph_layouts.py::test_catalogue_properties asserts)
CASES = [(name, fam) for name in gg.CATALOGUE for fam in FAMILIES if (name, fam) != ("lds_edge", "resident_k1")]


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


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """name of a catalogue graph, or (base, kind) of a near-T o LM graph -> dict(path, g, V, rest_rows, batches: tag -> logits, labels,
    lx, ly, sigma, den = the oracle's (gamma, log Z forward, log Z backward), ref[size_average] = oracle.ctc_crf): computed once per
    graph, read-only."""
    d = tmp_path_factory.mktemp("gpu_general_graphs")
    cache = {}

    def get(key):
        if key not in cache:
            from cat_amd.ctc_crf import _C as core
            if key in gg.CATALOGUE:
                path, g, V = gg.catalogue(key, d)
            else:
                _, path, g, V = gg.near_tolm_case(key[0], key[1], gg.SEEDS[0], d)
            h = core.compile_graph_host_only(path)
            rest = core.debug_stream_check(h, 8, 64)["rest_rows"]
            core._lib.crf_graph_destroy(ctypes.c_void_p(h))
            batches = {}
            for tag, sigma, lx, seed in gg.batches_of(key):
                logits, labels, lx, ly = gg.batch(V, sigma, seed, lx)
                den = oracle.den(g, logits, lx)
                assert np.isfinite(den[1]).all() and np.isfinite(den[2]).all(), (key, tag)
                ref = {sa: oracle.ctc_crf(g, logits, labels, lx, ly, lamb=LAMB, size_average=sa) for sa in (False, True)}
                batches[tag] = dict(logits=logits, labels=labels, lx=lx, ly=ly, sigma=sigma, den=dict(gamma=den[0], ca=den[1], cb=den[2]), ref=ref)
            cache[key] = frozen(dict(path=path, g=g, V=V, rest_rows=rest, batches=batches))
        return cache[key]
    return get


def run_and_hold(crf, case, tag, size_average, what, unused_from=None, no_fallback=False):
    """One batch on the graph loaded on the device: CTC_CRF_LOSS forward and backward, then gpu_den; every assertion of the module's
    docstring.  Returns (kernel, fallback counts, worst rel_err, worst post_err)."""
    core = crf._C
    bt = case["batches"][tag]
    logits, labels, lx, ly = bt["logits"], bt["labels"], bt["lx"], bt["ly"]
    ref, den = bt["ref"][size_average], bt["den"]
    x = torch.tensor(logits, device=DEV, requires_grad=True)
    loss = crf.CTC_CRF_LOSS(lamb=LAMB, size_average=size_average)(x, torch.tensor(labels, dtype=torch.int32), torch.tensor(lx, dtype=torch.int32),
                                                                  torch.tensor(ly, dtype=torch.int32))
    loss.backward()
    kernel = core.last_den_kernel()
    falls = core.last_fallback_counts(torch.cuda.current_stream().cuda_stream)
    loss, grad = float(loss.item()), x.grad.cpu().numpy()
    lg = torch.tensor(logits, device=DEV)
    gd, ca, cb = torch.zeros_like(lg), torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
    core.gpu_den(lg, gd, torch.tensor(lx, dtype=torch.int32).cuda(), ca, cb)       # (the den-only loss_fwd_bwd call: gamma_den and both log Z)
    kernel_den = core.last_den_kernel()
    gd, ca, cb = gd.cpu().numpy(), ca.cpu().numpy().astype(np.float64), cb.cpu().numpy().astype(np.float64)
    floor = 0.05 * (1.0 / B if size_average else 1.0)
    errs = [rel_err(grad[b], ref["grad"][b], floor) if lx[b] > 0 else 0.0 for b in range(B)]
    perrs = [post_err(gd[b, :lx[b]], den["gamma"][b, :lx[b]]) if lx[b] > 0 else 0.0 for b in range(B)]
    print(what, tag, "kernel", kernel, "| den-only", kernel_den, "fallbacks", falls, "loss", loss, "oracle", ref["loss"], "rel_err", errs, "post_err", perrs,
          "logZ", ca.tolist(), cb.tolist(), "oracle", den["ca"].tolist())
    assert np.isfinite(loss) and np.isfinite(grad).all() and np.isfinite(gd).all() and np.isfinite(ca).all() and np.isfinite(cb).all(), (what, tag)
    assert abs(loss - ref["loss"]) <= TOL * max(1.0, abs(ref["loss"])), (what, tag, loss, ref["loss"])
    for b in range(B):
        n = int(lx[b])
        assert errs[b] <= TOL, (what, tag, "gradient", b, errs[b])
        assert perrs[b] <= TOL, (what, tag, "gamma_den", b, perrs[b])
        assert abs(ca[b] - den["ca"][b]) <= TOL * max(1.0, abs(den["ca"][b])), (what, tag, "forward log Z", b, ca[b], den["ca"][b])
        assert abs(cb[b] - den["cb"][b]) <= TOL * max(1.0, abs(den["cb"][b])), (what, tag, "backward log Z", b, cb[b], den["cb"][b])
        assert np.all(grad[b, n:] == 0.0) and np.all(gd[b, n:] == 0.0), (what, tag, "frames past lx", b)
    if unused_from is not None:
        assert np.all(gd[:, :, unused_from:] == 0.0), (what, tag, "classes no arc carries")
    if no_fallback:
        assert falls == (0, 0), (what, tag, falls)
    return kernel, kernel_den, falls, max(errs), max(perrs)


def row(name, fam, tag, st, case, den_kernels, kernel, falls, err, perr):
    print(f"ROW | {name} | {fam} | {tag} | S={st['S']} A={st['A']} P={st['P']} | rows {st['res_fwd_rows']}/{st['res_bwd_rows']} | rest_rows={case['rest_rows']} | "
          f"res_K={st['res_K']} fac={st['fac']} | {den_kernels} | {kernel} | fallbacks {falls[0]},{falls[1]} | rel_err {err:.2e} | post_err {perr:.2e}")


def test_destroying_a_host_only_graph_leaves_no_hip_error(crf, golden_dir):
    """What this module's fixture found: crf_graph_destroy of a HOST-ONLY graph (device -1) called hipSetDevice(-1); the runtime kept
    hipErrorInvalidDevice as the thread's last error, and the next launch check -- torch's own, or the library's in crf_stage_i32 --
    reported "invalid device ordinal" for a call that had nothing wrong.  Both kinds of call right behind such a destroy."""
    import json
    import os
    core = crf._C
    k = json.load(open(os.path.join(golden_dir, "kat_fixture.json")))
    fst = os.path.join(golden_dir, "den_lm_fixture.fst")
    ctx = crf.CRFContext(fst, 0)
    logits = torch.tensor(np.log(np.array(k["probs"], dtype=np.float32))[None], device=DEV)
    for first in ("torch", "library"):
        h = core.compile_graph_host_only(fst)
        core._lib.crf_graph_destroy(ctypes.c_void_p(h))
        if first == "torch":
            assert float((logits * 0.0 + 1.0).sum().item()) == logits.numel()
        gd, ca, cb = torch.zeros_like(logits), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        core.gpu_den(logits, gd, torch.tensor([5], dtype=torch.int32), ca, cb)
        assert abs(ca.item() - k["logZ_den"]) <= TOL * abs(k["logZ_den"]) and abs(cb.item() - k["logZ_den"]) <= TOL * abs(k["logZ_den"])
    del ctx


@pytest.mark.parametrize("name,fam", CASES)
def test_general_graph(crf, refs, name, fam):
    core = crf._C
    case = refs(name)
    mode, switches, want_k, kernel_ok = FAMILIES[fam]
    size_average = bool((list(gg.CATALOGUE).index(name) + list(FAMILIES).index(fam)) % 2)
    with (_mode(mode) if mode else crf_env()), crf_env(**switches):
        ctx = crf.CRFContext(case["path"], 0)
        h = core.graph_for(DEV)
        st = core.graph_stats(h)
        dk = core.den_kernels(h, B, 40, case["V"])
        assert st["fac"] == 0 and st["S"] == case["g"]["S"] and st["A"] == case["g"]["A"], st
        if want_k is not None:
            assert st["res_K"] == want_k and dk == "resident", (name, fam, st["res_K"], dk)
        elif mode is not None:
            assert st["res_K"] == 0 and dk == ("streaming" if mode == "streaming" else "batch"), (name, fam, st["res_K"], dk)
        for tag in case["batches"]:
            if tag == "s2_lx0" and fam != "default":            # (the utterance of no frames: one case per graph)
                continue
            kernel, kernel_den, falls, err, perr = run_and_hold(
                crf, case, tag, size_average, (name, fam), unused_from=6 if name == "parallel" else None,
                no_fallback=case["batches"][tag]["sigma"] == 2.0 and name != "one_final")
            assert kernel_ok(kernel) and kernel_ok(kernel_den), (name, fam, tag, kernel, kernel_den)
            row(name, fam, tag, st, case, dk, kernel, falls, err, perr)
        del ctx


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", gg.KINDS)
@pytest.mark.parametrize("base", list(gg.BASES))
def test_near_tolm_graph(crf, refs, base, kind, mode):
    """A T o LM graph with three arcs changed in every mode of the parity tests: the factored kernels where the analysis still accepts the
    graph (with unmatched pairs and tail rows), a correct other family where it refuses it."""
    core = crf._C
    case = refs((base, kind))
    with _mode(mode):
        ctx = crf.CRFContext(case["path"], 0)
        h = core.graph_for(DEV)
        st = core.graph_stats(h)
        dk = core.den_kernels(h, B, 40, case["V"])
        if not mode.startswith("factored"):
            assert st["fac"] == 0, (mode, st)
        kernel, kernel_den, falls, err, perr = run_and_hold(crf, case, "s2", True, (base, kind, mode))
        for k in (kernel, kernel_den):
            assert k.startswith("crf_fac") == (st["fac"] == 1) and len(k) > 0, (base, kind, mode, st["fac"], k)
        assert (dk == "factored") == (st["fac"] == 1), (base, kind, mode, dk)
        row(f"{base}_{kind}", mode, "s2", st, case, dk, kernel, falls, err, perr)
        del ctx
