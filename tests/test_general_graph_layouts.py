"""Host-only checks (no GPU) of the graph compiler on graphs WITHOUT the T o LM structure and on T o LM graphs with a few arcs changed
(tests/general_graphs.py): the generic register-resident layout for K = 1, 2, 4 compute units walked on the host like the kernels walk
it (crf_debug_res_emulate, which checks the grad pass's pair lists too), the utterance-minor kernels' arc streams and their rest list
(crf_debug_stream_check), the factored layout where the analysis still accepts the graph (crf_debug_fac_emulate,
crf_debug_facbatch_check), and the property each catalogue graph is there for.  tests/test_gpu_general_graphs.py runs the same graphs
through the kernels.

The reference's own denominator is not run on `hub` here: tests/test_oracle.py has no helper that runs the binaries of oracle/_ref on a
graph file."""
import ctypes
import math

import numpy as np
import pytest

import oracle
from tests import general_graphs as gg
from tests.util import crf_env


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


@pytest.fixture(scope="module")
def graphs(tmp_path_factory):
    d = tmp_path_factory.mktemp("general_graphs")
    return {name: gg.catalogue(name, d) for name in gg.CATALOGUE}


@pytest.fixture(scope="module")
def near(tmp_path_factory):
    d = tmp_path_factory.mktemp("near_tolm")
    return {(b, kind, seed): gg.near_tolm_case(b, kind, seed, d) for b in gg.BASES for kind in gg.KINDS for seed in gg.SEEDS}


def agree(r):
    """The rule of tests/test_abi.py::test_generic_resident_layout_emulated_on_the_host."""
    return all(math.isfinite(x) and x > 0 for x in r) and abs(r[1] - r[0]) <= 1e-9 * r[0] and abs(r[2] - r[0]) <= 1e-6 * r[0]


class host_graph:
    def __init__(self, core, path, **env):
        self.core, self.path, self.env = core, path, crf_env(**env)

    def __enter__(self):
        self.env.__enter__()
        self.h = self.core.compile_graph_host_only(self.path)
        return self.h

    def __exit__(self, *a):
        self.core._lib.crf_graph_destroy(ctypes.c_void_p(self.h))
        return self.env.__exit__(*a)


def entering_labels(g):
    """Per state: how many distinct classes enter it."""
    pairs = np.unique(np.stack([g["dst"], g["lab"]], 1), axis=0)
    return np.bincount(pairs[:, 0], minlength=g["S"])


@pytest.mark.parametrize("mink", [1, 2, 4])
@pytest.mark.parametrize("name", list(gg.CATALOGUE))
def test_generic_layout_and_streams_of_general_graphs(core, graphs, name, mink):
    path, g, V = graphs[name]
    with host_graph(core, path, CRF_NO_FACTORED=1, CRF_RES_MINK=mink) as h:
        st = core.graph_stats(h)
        assert st["fac"] == 0 and st["res_K"] == mink, (name, st)
        assert st["S"] == g["S"] and st["A"] == g["A"]
        for T in (1, 2, 5):
            r = core.debug_res_emulate(h, T, 11 + T)
            assert agree(r), (name, mink, T, r)
        for UL in (8, 64):
            s4 = core.debug_stream_check(h, UL, 64)
            print(name, "K", mink, "UL", UL, "P", st["P"], s4)
            # what sets these graphs apart from T o LM ones, whose rest list holds at most two rows
            assert s4["rest_rows"] >= st["P"] // 4, (name, UL, s4, st["P"])


def test_catalogue_properties(core, graphs):
    """The property each catalogue graph must have, from crf_graph_stats / crf_graph_dims (and, where they do not report it, from the
    arcs)."""
    stats = {}
    for name, (path, g, V) in graphs.items():
        with host_graph(core, path, CRF_NO_FACTORED=1) as h:
            stats[name] = (core.graph_stats(h), core.graph_dims(h), core.den_kernels(h, 4, 30, V))
        S, live_final = g["S"], np.isfinite(g["end_w"])
        out_deg, in_deg = np.bincount(g["src"], minlength=S), np.bincount(g["dst"], minlength=S)
        kw = gg.CATALOGUE[name][1]
        live = S - kw.get("dead", 0) - kw.get("unreach", 0)
        # the generator's guarantees: dead ends, unreachable states, the start, a final state one ring step away with a self loop
        assert g["start"] == kw["start"] and live_final[(kw["start"] + 1) % live]
        assert np.any((g["src"] == (kw["start"] + 1) % live) & (g["dst"] == (kw["start"] + 1) % live))
        dead = np.arange(live, live + kw.get("dead", 0))
        unre = np.arange(live + kw.get("dead", 0), S)
        assert np.all(out_deg[dead] == 0) and np.all(in_deg[dead] > 0) and not live_final[dead].any()
        assert np.all(in_deg[unre] == 0) and np.all(out_deg[unre] > 0)
        assert np.all(g["dst"][np.isin(g["src"], unre)] < live)
        print(name, stats[name])
    st, dims, _ = stats["multi"]
    assert st["P"] > st["S"] and st["res_K"] == 1 and entering_labels(graphs["multi"][1]).max() > 1
    st, dims, _ = stats["hub"]
    g = graphs["hub"][1]
    assert st["max_in_deg"] >= 300 and st["max_out_deg"] >= 300
    assert st["res_fwd_rows"] > st["P"]                         # sub-rows exist ...
    _, n = np.unique(np.stack([g["dst"], g["lab"]], 1), axis=0, return_counts=True)
    assert n.max() >= 300                                       # ... they must: 300 arcs of ONE class enter one state, a row holds 96
    st, dims, _ = stats["wide"]
    assert st["res_fwd_rows"] >= 5000 and st["res_K"] == 1
    st, dims, kern = stats["lds_edge"]
    assert st["res_K"] == 1 and kern != "resident"              # a K = 1 layout exists, and its rows do not fit the LDS at V = 72
    path, g, V = graphs["lds_edge"]
    with host_graph(core, path, CRF_NO_FACTORED=1, CRF_RES_MINK=2) as h:
        assert core.graph_stats(h)["res_K"] == 2 and core.den_kernels(h, 4, 30, V) == "resident"
    with host_graph(core, path) as h:                           # by default too, and at the GPU tests' T = 40 (which leave K = 1 out for this graph)
        assert core.graph_stats(h)["res_K"] == 1 and core.den_kernels(h, 4, 30, V) != "resident" and core.den_kernels(h, 4, 40, V) != "resident"
    st, dims, _ = stats["parallel"]
    g = graphs["parallel"][1]
    assert dims["max_label"] == 5 and graphs["parallel"][2] == 12
    assert entering_labels(g).max() >= 6
    assert set(g["src"][g["src"] == g["dst"]]) == set(g["src"]) and g["start"] in set(g["src"])   # a self loop on every state that has arcs
    arcs, n = np.unique(np.stack([g["src"], g["dst"], g["lab"]], 1), axis=0, return_counts=True)
    assert n.max() >= 2                                         # duplicated arcs
    _, n = np.unique(arcs[:, :2], axis=0, return_counts=True)
    assert n.max() == 6                                         # a (src, dst) pair joined by all six classes
    g = graphs["one_final"][1]
    cost = -g["w"]
    assert np.isfinite(g["end_w"]).sum() == 1 and cost.min() >= 0.0 and 6.0 < cost.max() <= 12.0
    for name in gg.CATALOGUE:                                   # the fallback counts are asserted on graphs with costs <= 2
        if name != "one_final":
            assert -graphs[name][1]["w"].min() <= 2.0 and -graphs[name][1]["end_w"][np.isfinite(graphs[name][1]["end_w"])].min() <= 2.0


CONFIGS = [{}, dict(CRF_FAC_THREADS=768), dict(CRF_FAC_K2=1), dict(CRF_NO_FACTORED=1)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "fac_threads_768", "fac_k2", "no_factored"])
def test_near_tolm_graphs_keep_a_correct_layout(core, near, cfg):
    """T o LM graphs with three arcs deleted, re-weighted, duplicated, added, relabelled or redirected: whichever layouts the compiler
    reports are walked on the host and must agree with the plain recursion; where the factored layout survives, the factored rows and
    streams of the utterance-minor kernels are checked too.  Both outcomes occur for each base graph: the factored layout kept with
    fewer matched pairs than the base graph has, and the factored layout refused."""
    kept, lost = set(), set()
    base_pairs = {}
    for (b, kind, seed), (bp, p, g, V) in near.items():
        if b not in base_pairs:
            with host_graph(core, bp, **cfg) as h:
                st = core.graph_stats(h)
                assert st["fac"] == (0 if "CRF_NO_FACTORED" in cfg else 1), (b, st)
                base_pairs[b] = st["fac_matched_pairs"]
        with host_graph(core, p, **cfg) as h:
            st = core.graph_stats(h)
            assert st["fac"] == 1 or st["res_K"] >= 1, (b, kind, seed, st)
            if st["fac"] == 1:
                r = core.debug_fac_emulate(h, 5, 7)
                assert agree(r), ("factored", b, kind, seed, r)
                chk = core.debug_facbatch_check(h)
                s4 = core.debug_stream_check(h, -16, 64)
                assert chk["NU"] > 0 and chk["arcs"] == st["A"] and s4["tasks"] >= 2, (b, kind, seed, chk, s4)
                if st["fac_matched_pairs"] < base_pairs[b]:
                    kept.add(b)
            else:
                lost.add(b)
            if st["res_K"] >= 1:
                r = core.debug_res_emulate(h, 5, 7)
                assert agree(r), ("generic", b, kind, seed, r)
            print(b, kind, seed, cfg, "fac", st["fac"], "matched", st["fac_matched_pairs"], "of", base_pairs[b], "res_K", st["res_K"])
    if "CRF_NO_FACTORED" in cfg:
        assert not kept and lost == set(gg.BASES)
    else:
        assert kept == set(gg.BASES) and lost == set(gg.BASES), (kept, lost)


def test_every_utterance_of_the_gpu_batches_has_paths(graphs, near):
    """Z > 0: the oracle's log Z is finite for every utterance of every batch tests/test_gpu_general_graphs.py runs -- which is what
    lets those tests run every case."""
    cases = [(name, g, V) for name, (p, g, V) in graphs.items()] + [(key, g, V) for key, (bp, p, g, V) in near.items() if key[2] == gg.SEEDS[0]]
    for name, g, V in cases:
        for tag, sigma, lx, seed in gg.batches_of(name):
            logits, labels, lx, ly = gg.batch(V, sigma, seed, lx)
            assert ly.max() > 0 and ly.min() == 0 and np.all(ly <= lx // 3)
            gamma, ca, cb = oracle.den(g, logits, lx)
            assert np.isfinite(ca).all() and np.isfinite(cb).all() and np.isfinite(gamma).all(), (name, tag, ca, cb)
            _, cc, valid = oracle.ctc(logits, labels, lx, ly)
            assert valid.all() and np.isfinite(cc).all(), (name, tag)
