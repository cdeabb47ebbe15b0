"""GPU test: crf_ctc_edit_distance through the C ABI on buffers carved from a guard-banded arena (tests/guard.py), as
tests/test_gpu_beam_guard_bands.py does for the beam search -- hyp_stride larger than any row's use, the references exactly as long as
their lengths say, ops_dev NULL and non-NULL, every kernel instantiation.  There is no workspace.  No byte outside the call's own buffers
may change, no input may change, every output word must be written, and the results equal the yardstick."""
import ctypes

import numpy as np
import pytest
import torch

from tests import edit_ref
from tests.guard import Arena

pytestmark = pytest.mark.gpu
SENT = -77


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf._C


def run_edit(core, rows, lens, utt, refs, with_ops):
    """rows: CPU int32 [H, stride].  -> (dist [H], ops [H, 3] or None) as numpy after the guard check."""
    dev = torch.device("cuda", 0)
    H, stride = rows.shape
    B = len(refs)
    lab = torch.tensor([t for r in refs for t in r], dtype=torch.int32)
    ly = torch.tensor([len(r) for r in refs], dtype=torch.int32)
    off = torch.cumsum(ly, 0, dtype=torch.int32) - ly
    ins = (("hyps", rows), ("hyp_len", torch.tensor(lens, dtype=torch.int32)), ("hyp_utt", torch.tensor(utt, dtype=torch.int32)), ("refs", lab),
           ("ref_off", off), ("ref_len", ly))
    arena = Arena(dev, Arena.room([4 * t.numel() for _, t in ins] + [4 * H, 12 * H]))
    for name, t in ins:
        arena.carve(name, 4 * t.numel())
        arena.put(name, t)
    for name, n in (("dist", H),) + ((("ops", 3 * H),) if with_ops else ()):
        arena.carve(name, 4 * n)
        arena.put(name, torch.full((n,), SENT, dtype=torch.int32))
    P, vp = arena.ptr, ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        rc = core._lib.crf_ctc_edit_distance(P("hyps"), stride, P("hyp_len"), P("hyp_utt"), P("refs"), P("ref_off"), P("ref_len"), B, H,
                                             int(ly.max()), P("dist"), P("ops") if with_ops else vp(0), stream)
    assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check()
    for name, t in ins:
        assert torch.equal(arena.get(name, torch.int32), t.reshape(-1)), f"the call wrote to {name}"
    dist = arena.get("dist", torch.int32).numpy()
    ops = arena.get("ops", torch.int32, (H, 3)).numpy() if with_ops else None
    assert not np.any(dist == SENT) and (ops is None or not np.any(ops == SENT))
    return dist, ops


@pytest.mark.parametrize("max_ref,kernel", [(64, "<1>"), (100, "<2>"), (256, "<4>"), (300, "<8>"), (700, "<8, strips>")])
def test_edit_writes_only_its_own_memory(core, max_ref, kernel):
    rng = np.random.default_rng(max_ref)
    refs = [rng.integers(1, 4, n).tolist() for n in (max_ref, 1, max_ref - 3)]     # the last reference ends with the buffer
    stride, used = 200, 130                                                        # rows wider than any hypothesis
    utt = [2, 0, 1, 2, 0, 7, 1]                                                    # H = 7; row 5 names no utterance
    lens = [used, 65, 0, 1, 64, 10, -3]                                            # ... and row 6 has no length
    rows = torch.tensor(rng.integers(1, 4, (len(utt), stride)), dtype=torch.int32)
    hyps = [rows[h, :n].tolist() if 0 <= u < 3 and n >= 0 else None for h, (u, n) in enumerate(zip(utt, lens))]
    want = np.full((len(utt), 4), -1, dtype=np.int64)
    for h, y in enumerate(hyps):
        if y is not None:
            want[h] = edit_ref.antidiag(refs[utt[h]], y)
    for with_ops in (False, True):
        dist, ops = run_edit(core, rows, lens, utt, refs, with_ops)
        assert core.last_edit_kernel() == "crf_ctc_edit_kernel" + kernel
        assert np.array_equal(dist, want[:, 0])
        if with_ops:
            assert np.array_equal(ops, want[:, 1:])
