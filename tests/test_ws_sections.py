"""CPU tests (no GPU) of the workspace's section map (crf_debug_ws_sections, crf_debug_align_ws_sections, the switch ws_gap) on host-only
graphs of every kernel family, of the packed layout against the totals recorded from the commit before the map existed
(tests/golden/ws_totals.json; tests/golden/make_ws_totals.py regenerates it), and of the guard-band checker of tests/guard.py itself."""
import json
import os

import pytest
import torch

from tests.conftest import ROOT
from tests.guard import GUARD, Arena, GuardError
from tests.test_gpu_parity import MODES, _mode
from tests.util import crf_env, small_synth

# (B, T, labels L, bat_ul): B = 1, odd B, B = 9 in groups of 8 (seven padding utterances), no labels at all, the staged schedule's T
SHAPES = [(1, 20, 3, 0), (5, 37, 6, 0), (9, 31, 5, 8), (4, 300, 0, 0), (3, 64, 10, 0), (64, 50, 8, 0)]
ALIGN_SHAPES = [(1, 1, 5, 0), (3, 35, 37, 0), (3, 35, 257, 31), (3, 35, 257, 32), (7, 100, 8192, 2047)]
GOLDEN = os.path.join(ROOT, "tests", "golden", "ws_totals.json")


def graph_files(tmp):
    """name -> (file, V, modes): the T o LM graph of the utterance-group tests, the S = 513 graph of tests/test_gpu_schedules.py, a general
    graph (states entered with several labels: no factored layout), and -- streaming only -- the S = 20 001 graph of
    test_large_graph_global_vectors, whose state vectors live in the workspace (section gvec)."""
    from cat_amd.den_lm import synth_den_lm
    p513, pbig = os.path.join(str(tmp), "s513.fst"), os.path.join(str(tmp), "big.fst")
    synth_den_lm(72, 256, 16, 0, path=p513)
    synth_den_lm(72, 10000, 8, seed=3, path=pbig)
    return {"synth12": (small_synth(tmp, 12, 40, 6, 5)[1], 12, MODES), "s513": (p513, 72, MODES),
            "general": (os.path.join(ROOT, "tests", "golden", "rand2.fst"), 9, MODES), "s20001": (pbig, 72, ["streaming"])}


def matrix(core, tmp):
    """Yields (key, handle or None, B, T, V, L, bat_ul) with the mode's switches set: every graph x every parity mode x SHAPES, and the
    numerator-only calls (no graph).  The handles are host-only graphs."""
    for gname, (path, V, modes) in graph_files(tmp).items():
        for mode in modes:
            with _mode(mode):
                h = core.compile_graph_host_only(path)
                for B, T, L, ul in SHAPES:
                    with crf_env(**({"CRF_BAT_UL": ul} if ul else {})):
                        yield f"{gname}|{mode}|{B},{T},{V},{L}|{ul}", h, B, T, V, L, ul
                core._lib.crf_graph_destroy(h)
    for B, T, L, ul in SHAPES:
        yield f"none|-|{B},{T},37,{L}|0", None, B, T, 37, L, 0


def totals(core, tmp):
    """key -> crf_workspace_bytes / crf_ctc_align*_workspace_bytes, for the golden file (needs nothing newer than those three exports)."""
    out = {key: int(core._lib.crf_workspace_bytes(h, B, T, V, L)) for key, h, B, T, V, L, _ in matrix(core, tmp)}
    for B, T, V, L in ALIGN_SHAPES:
        out[f"align|{B},{T},{V},{L}"] = int(core._lib.crf_ctc_align_workspace_bytes(B, T, V, L))
        out[f"align_logits|{B},{T},{V},{L}"] = int(core._lib.crf_ctc_align_logits_workspace_bytes(B, T, V, L))
    return out


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def check_map(secs, total, what):
    assert secs[0][1] == 0, what
    end = 0
    for name, off, nb in secs:
        assert off % 256 == 0 and nb >= 0 and off >= end, (what, name, off, nb, end)   # 256-aligned, ascending, disjoint
        end = off + nb
    assert end <= total, (what, end, total)


def test_section_map_and_gap(core, tmp_path):
    names = [s[0] for s in core.debug_ws_sections(None, 1, 1, 2, 0)]
    assert core._lib.crf_debug_ws_section_names().decode().split(",") == names
    seen_sizes = {}
    n = 0
    for key, h, B, T, V, L, _ in matrix(core, tmp_path):
        secs = core.debug_ws_sections(h, B, T, V, L)
        total = core._lib.crf_workspace_bytes(h, B, T, V, L)
        assert [s[0] for s in secs] == names and len(set(names)) == len(names) >= 20
        check_map(secs, total, key)
        # packed: the next section starts at the next multiple of 256 behind this one, the total behind the last
        for k, (name, off, nb) in enumerate(secs):
            nxt = secs[k + 1][1] if k + 1 < len(secs) else total
            assert nxt == (off + nb + 255) // 256 * 256, (key, name)
            if nb:
                seen_sizes.setdefault(name, set()).add(nb)
        for gap in (1, 3):
            with core.debug_opts(ws_gap=gap):
                gsecs = core.debug_ws_sections(h, B, T, V, L)
                gtotal = core._lib.crf_workspace_bytes(h, B, T, V, L)
            check_map(gsecs, gtotal, (key, gap))
            assert [(nm, off + gap * 256 * k, nb) for k, (nm, off, nb) in enumerate(secs)] == gsecs, (key, gap)
            assert gtotal == total + gap * 256 * len(secs), (key, gap)
        n += 1
    assert n == (3 * len(MODES) + 2) * len(SHAPES)
    # the matrix reaches every section -- each has a size > 0 somewhere, the family-specific ones in their family -- but those of the
    # utterance-minor kernels: a host-only graph has no tables for them (tests/test_gpu_guard_bands.py has them, on the device)
    assert set(names) - set(seen_sizes) == {"ept", "Af", "Zb", "bsm"}, set(names) - set(seen_sizes)


def test_align_section_map_and_gap(core):
    assert [s[0] for s in core.debug_align_ws_sections(True, 1, 1, 2, 0)] == ["bp", "lse"]
    assert core._lib.crf_debug_align_ws_section_names().decode() == "bp,lse"
    for B, T, V, L in ALIGN_SHAPES:
        for logits, fn in ((False, core._lib.crf_ctc_align_workspace_bytes), (True, core._lib.crf_ctc_align_logits_workspace_bytes)):
            secs, total = core.debug_align_ws_sections(logits, B, T, V, L), fn(B, T, V, L)
            assert [s[0] for s in secs] == (["bp", "lse"] if logits else ["bp"])
            check_map(secs, total, (B, T, V, L, logits))
            assert secs[0][2] == B * ((T + 15) // 16) * ((2 * L + 1 + 63) // 64 * 64) * 4
            if logits:
                assert secs[1][2] == B * T * 4
            with core.debug_opts(ws_gap=2):
                gsecs, gtotal = core.debug_align_ws_sections(logits, B, T, V, L), fn(B, T, V, L)
            assert [(nm, off + 512 * k, nb) for k, (nm, off, nb) in enumerate(secs)] == gsecs
            assert gtotal == total + 512 * len(secs)
    with pytest.raises(RuntimeError):
        core.debug_align_ws_sections(False, 2, 10, 8193, 3)


def test_default_layout_unchanged(core, tmp_path):
    """With ws_gap unset the totals are those of the commit before the section map, for the whole matrix."""
    want = json.load(open(GOLDEN))
    got = totals(core, tmp_path)
    assert set(got) == set(want)
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, diff


def test_checker_names_the_corrupted_band():
    """The negative control of tests/guard.py: a byte flipped by a torch write in a guard band, and one in a gap between two sections."""
    arena = Arena(torch.device("cpu"), Arena.room([1000, 6, 2048]))
    a = arena.carve("a", 1000)
    b = arena.carve("b", 6, misalign=2)
    ws = arena.carve("ws", 2048)
    assert a.data_ptr() % 256 == 0 and b.data_ptr() % 256 == 2 and ws.data_ptr() % 256 == 0
    assert b.data_ptr() - (a.data_ptr() + 1000) >= 2 * GUARD
    a.fill_(0); b.fill_(1); ws.fill_(2)                      # writing every byte of the buffers themselves is fine
    secs = [("s0", 0, 100), ("s1", 256, 0), ("s2", 512, 700), ("s3", 1280, 256)]   # (s1 is empty; a gap of 512 behind s3)
    ws.fill_(0xFF)
    for name, off, nb in secs:
        ws[off:off + nb] = 7
    arena.check()
    arena.check(secs)
    start = {n: arena.carves[n][0] for n in arena.carves}
    cases = [(start["a"] + 1000 + 5, 1, "a", "after", 1005, 1005), (start["b"] - 3, 2, "b", "before", -3, -2),
             (start["a"] - 1, 1, "a", "before", -1, -1), (start["ws"] + 2048 + GUARD - 1, 1, "ws", "after", 2047 + GUARD, 2047 + GUARD),
             (start["ws"] + 100, 1, "ws.s0", "after", 100, 100), (start["ws"] + 300, 4, "ws.s1", "after", 44, 47),
             (start["ws"] + 1279, 1, "ws.s2", "after", 767, 767), (start["ws"] + 2047, 1, "ws.s3", "after", 767, 767)]
    for at, n, name, side, first, last in cases:
        arena.buf[at:at + n] = 0
        with pytest.raises(GuardError) as e:
            arena.check(secs)
        assert (e.value.name, e.value.side, e.value.first, e.value.last) == (name, side, first, last), str(e.value)
        assert name in str(e.value) and side in str(e.value) and str(first) in str(e.value)
        if not name.startswith("ws."):
            with pytest.raises(GuardError):
                arena.check()
        else:
            arena.check()                                    # without the map the inside of the workspace is not looked at
        arena.buf[at:at + n] = 0xFF
        arena.check(secs)
    with pytest.raises(AssertionError):                      # a map whose sections overlap is refused
        arena.check([("s0", 0, 300), ("s1", 256, 10)])
