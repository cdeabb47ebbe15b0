"""CPU test (no GPU) of the INPUTS of tests/test_gpu_ctc_score_grad_logits.py, with the fp64 reference alone: every parity case
(tests/score_grad_logits_ref.py: PARITY_CASES) is in the regime its tolerance is meant for.  These are conditions on the references, not
measurements of a kernel.

  scale    the reference gradient's largest entry is at least 0.05 x the largest sum over an utterance's live hypotheses of |w_h| -- the
           floor convention of tests.util.rel_err: the gradient is the difference of two terms of that scale (the folded occupancies and
           W_u softmax), and 1e-4 of its largest entry is then no demand on their cancellation noise.
  mixed    with weights of mixed sign the reference keeps at least 0.1 of the norm of its twin under the absolute weights, as
           tests/test_gpu_ctc_score_grad.py asserts of its small case."""
import numpy as np
import pytest

from tests.score_grad_logits_ref import PARITY_CASES, fold_raw, live_weight, parity_case

SCALE, MIXED = 0.05, 0.1


@pytest.mark.parametrize("name", list(PARITY_CASES))
def test_parity_case_is_in_its_regime(name):
    c = parity_case(name)
    r = c["ref"]
    N = c["x32"].shape[0]
    assert r["live"].any() and np.all(np.isfinite(r["cost"][r["live"]]))
    assert np.all(np.isfinite(c["x32"]).any(-1)), "every row keeps a finite entry"
    for wname, w in c["weights"].items():
        ref = fold_raw(r, c["utt"], w, c["lx"])
        scale = live_weight(r, c["utt"], w, N, absolute=True).max()
        print(f"[score_grad_logits inputs] {name} w={wname}: max |ref| {np.abs(ref).max():.3e}, scale {scale:.3e}")
        assert np.all(np.isfinite(ref)) and np.abs(ref).max() >= SCALE * scale, (name, wname, float(np.abs(ref).max()), scale)
        if w is not None and np.any(np.asarray(w) < 0):
            twin = fold_raw(r, c["utt"], np.abs(w), c["lx"])
            print(f"[score_grad_logits inputs] {name} w={wname}: norm {np.linalg.norm(ref):.3e} of the absolute-weight twin's {np.linalg.norm(twin):.3e}")
            assert np.linalg.norm(ref) >= MIXED * np.linalg.norm(twin), (name, wname)
