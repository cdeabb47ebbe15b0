"""CPU test (no GPU) of the INPUTS of tests/test_gpu_ctc_score_grad_uneven.py, with the fp64 oracle alone: every uneven case
(tests/score_grad_ref.py: UNEVEN_CASES) is in the regime it was built for.  These are conditions on the inputs, not measurements of a kernel.

  regime   the forward vector's largest entry leaves the straight ramp (t + 1) * cost / lx by at least 2 500 nats somewhere.  One fp32
           rounding of a value of that size is 2^-13 = 1.2e-4 and differs from state to state, so a forward vector stored in fp32
           relative to that ramp cannot give posteriors to 1e-4; emulated in fp64 with that one rounding, the entry-wise error crosses
           1e-4 where the distance is about 1 900.
  support  the reference has at least 50 posteriors >= 1e-3 (what tests.util.post_err looks at) in the 100 frames after each change
           of phase, where that distance is largest."""
import numpy as np
import pytest

import oracle
from tests.score_grad_ref import UNEVEN_CASES, flat, uneven_case

REGIME_NATS = 2500.0
SUPPORT_FRAMES, SUPPORT_ENTRIES = 100, 50


@pytest.mark.parametrize("name", list(UNEVEN_CASES))
def test_uneven_case_is_in_its_regime(name):
    c = uneven_case(name)
    assert c["blank"] == 0                                    # (oracle.ctc_alpha's own convention)
    assert np.all(c["valid"] == 1) and np.all(np.isfinite(c["cost"])), (c["valid"], c["cost"])
    assert len(c["hyps"][2]) == 0 and c["lx"][1] == 700 and np.all(c["w_pos"] > 0)
    lx = int(c["lx"][0])
    hyp = c["hyps"][0]
    _, cost, valid, alpha = oracle.ctc_alpha(c["logp"][:1], flat([hyp]), np.array([lx], dtype=np.int32), np.array([len(hyp)], dtype=np.int32))
    assert valid[0] == 1 and abs(cost[0] - c["cost"][0]) <= 1e-9 * abs(cost[0])
    top = np.nanmax(np.where(np.isfinite(alpha[0, :lx]), alpha[0, :lx], -np.inf), axis=1)
    assert np.all(np.isfinite(top))
    off = top - (np.arange(lx) + 1) * cost[0] / lx
    print(f"[uneven inputs] {name}: cost {cost[0]:.1f}, distance to the ramp {off.min():.0f} .. {off.max():.0f}")
    assert np.abs(off).max() >= REGIME_NATS, (name, float(np.abs(off).max()))
    if len(c["change"]) > 1:                                  # three phases: the distance changes sign
        assert off.max() >= REGIME_NATS and off.min() <= -REGIME_NATS, (name, off.min(), off.max())
    for t in c["change"]:
        n = int(np.sum(c["gamma"][0, t:t + SUPPORT_FRAMES] >= 1e-3))
        print(f"[uneven inputs] {name}: {n} posteriors >= 1e-3 in frames {t} .. {t + SUPPORT_FRAMES - 1}")
        assert n >= SUPPORT_ENTRIES, (name, t, n)
