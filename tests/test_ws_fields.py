"""CPU tests (no GPU) of what the loss call's host side decides before it lays the workspace down and of the arrays inside three of its
sections.

The field map (crf_debug_ws_fields): the sections pb, xch and bsm are carved from one field list each, and every pointer of the kernels'
parameter blocks into them is looked up in that list by name.  The expected offsets below were written down from the layout the host
carved by hand before the lists existed (they are multiples of B, or of Bp for bsm), not read from the code under test.

The denominator family (crf_den_kernels = choose_den_family): tests/golden/den_kernels.json holds what the library of the commit before
DenFamily answered -- there the family was a side effect of laying the workspace down -- for the graph files and MODES of
tests/test_ws_sections.py and B in {1, 9, 64, 200}.  To regenerate it, build that commit's library in a scratch checkout, then from this
repository's root:
    CRF_LIB=<scratch>/cat_amd/lib/libctc_crf_hip.so python -m tests.test_ws_fields
"""
import json
import os

import pytest

from tests.conftest import ROOT
from tests.test_gpu_parity import _mode
from tests.test_ws_sections import graph_files

GOLDEN = os.path.join(ROOT, "tests", "golden", "den_kernels.json")
K = 4   # kResMaxK

# section -> [(field, first byte as (multiple of n, constant), element bytes)]; n = B (bsm: Bp).  cb_F follows cb_part [B][kResMaxK].
PB = [("ctc_zc", (0, 0), 8), ("cb_mxs", (8, 0), 8), ("den_zs", (16, 0), 4), ("den_ez", (20, 0), 4), ("ctc_ez", (24, 0), 4),
      ("cost_alpha", (28, 0), 4), ("cost_beta", (32, 0), 4), ("cost_ctc", (36, 0), 4), ("invalid", (40, 0), 4), ("cb_part", (48, 0), 4),
      ("cb_F", (48 + 4 * K, 0), 4), ("redo", (80, 0), 4), ("redo_ctc", (88, 0), 4), ("ctc_logdom", (92, 0), 4)]
# bsm in bytes (4-byte words): mxf 0, mxb 3 Bp, Ef 6 Bp, Fb 7 Bp, zs 8 Bp, zb 9 Bp, bar 12 Bp.  The time-out word (BatchParams::err) is word
# 512 of `bar`, not a field of its own: crf_batch_init_kernel clears 640 words through `bar`, so the 512 barrier words, the time-out
# word and the 127 words behind it are ONE field.
BSM = [("mxf", (0, 0), 4), ("mxb", (12, 0), 4), ("Ef", (24, 0), 4), ("Fb", (28, 0), 4), ("zs", (32, 0), 4), ("zb", (36, 0), 4), ("bar", (48, 0), 4)]
XCH = [("flags", (0, 0), 4)]     # 64 flag words behind the granules, then 8 B spare bytes
# bytes the kernels index from a field's pointer: [B] unless noted ([3][Bp] maxima, [B][kResMaxK], [2][B]; 640 words cleared through bar)
EXTENT = {"cb_part": (4 * K, 0), "redo": (8, 0), "mxf": (12, 0), "mxb": (12, 0), "bar": (0, 640 * 4), "flags": (0, 64 * 4)}
SIZE = {"pb": (256, 0), "bsm": (48, 640 * 4), "xch": (8, 256)}


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def check_fields(core, section, n, want):
    f = core.debug_ws_fields(section, n)
    names = [x[0] for x in f]
    assert len(set(names)) == len(names), names
    end = 0
    for name, off, nb, elem in f:
        assert off >= end and nb >= 0 and off % elem == 0 and nb % elem == 0, (section, n, name, off, nb, elem, end)   # ascending, disjoint, aligned
        end = off + nb
    assert end == SIZE[section][0] * n + SIZE[section][1], (section, n, end)
    at = {x[0]: x for x in f}
    for name, (a, c), elem in want:
        _, off, nb, el = at[name]
        ea, ec = EXTENT.get(name, (elem, 0))
        assert off == a * n + c and el == elem and nb >= ea * n + ec, (section, n, name, off, nb, el)
    assert all(x.startswith("spare") for x in set(names) - {w[0] for w in want}), names
    return end


@pytest.mark.parametrize("B", [1, 5, 64])
def test_pb_and_xch_fields(core, B, tmp_path):
    pb, xch = check_fields(core, "pb", B, PB), check_fields(core, "xch", B, XCH)
    # ... and they end at or before the bytes crf_debug_ws_sections reports for the same call: no graph, a one-CU and a two-CU layout (the
    # fields of xch are the last bytes of the section, behind the granules)
    calls = [(None, 37)]
    hs = []
    for gname, mode in (("s513", "factored"), ("s513", "factored_k2"), ("general", "resident")):
        path, V, _ = graph_files(tmp_path)[gname]
        with _mode(mode):
            hs.append(core.compile_graph_host_only(path))
        calls.append((hs[-1], V))
    granules = set()
    for h, V in calls:
        secs = {s[0]: s[2] for s in core.debug_ws_sections(h, B, 40, V, 6)}
        assert pb <= secs["pb"] and xch <= secs["xch"] and (secs["xch"] - xch) % 256 == 0, (B, V, secs)
        granules.add(secs["xch"] - xch > 0)
    assert granules == {False, True}
    for h in hs:
        core._lib.crf_graph_destroy(h)
    with core.debug_opts(ws_gap=3):              # the switch acts between sections only
        assert check_fields(core, "pb", B, PB) == pb


@pytest.mark.parametrize("Bp", [8, 64])
def test_bsm_fields(core, Bp):
    # (a host-only graph has no utterance-minor tables, so no CPU call has a bsm section: its bytes are the list's, (12 Bp + 640) * 4,
    # which tests/test_gpu_guard_bands.py holds the kernels to on the device)
    assert check_fields(core, "bsm", Bp, BSM) == (12 * Bp + 640) * 4


def test_unknown_section(core):
    with pytest.raises(RuntimeError):
        core.debug_ws_fields("ep", 4)


def den_kernels_matrix(core, tmp):
    out = {}
    for gname, (path, V, modes) in graph_files(tmp).items():
        for mode in modes:
            with _mode(mode):
                h = core.compile_graph_host_only(path)
                for B in (1, 9, 64, 200):
                    out[f"{gname}|{mode}|{B}"] = core.den_kernels(h, B, 50, V)
                core._lib.crf_graph_destroy(h)
    return out


def test_den_kernels_are_the_parents(core, tmp_path):
    want = json.load(open(GOLDEN))
    got = den_kernels_matrix(core, tmp_path)
    assert set(got) == set(want)
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, diff
    assert {"streaming", "resident", "factored"} <= set(want.values())


if __name__ == "__main__":
    import tempfile

    import ctc_crf
    print("library:", ctc_crf._C.LIB_PATH)
    with tempfile.TemporaryDirectory() as tmp_dir:
        res = den_kernels_matrix(ctc_crf._C, tmp_dir)
    with open(GOLDEN, "w") as fh:
        json.dump(res, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(len(res), "answers ->", GOLDEN)
