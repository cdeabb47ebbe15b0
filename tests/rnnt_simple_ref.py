"""The yardstick of the rnnt_loss_simple tests (a plain helper module), numpy fp64 on top of tests/rnnt_ref.py: the joint tensor
x = f[:, :, None, :] + g[:, None, :, :] is formed here -- on the inputs' exact (already quantised) values -- and handed to the yardstick of
rnnt_loss on raw joiner output; the gradients of f and g are the joint gradient summed over u and over t."""
import numpy as np

from tests import rnnt_ref


def batch_ref(f, g, labels, lx, ly, blank):
    """f [N, T, V], g [N, U1, V] (fp64-able), labels [N, U1 - 1] -> (costs [N], d f like f, d g like g), zeros over the padding."""
    f, g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
    x = f[:, :, None, :] + g[:, None, :, :]
    costs, gx = rnnt_ref.batch_ref(x, labels, lx, ly, blank, True)
    return costs, gx.sum(2), gx.sum(1)


def random_case(seed, T_n, U_n, V, blank=0, T=None, U1=None, scale=3.0):
    """Padded raw f [N, T, V] and g [N, U1, V] fp32 and labels [N, U1 - 1] int32 without the blank; lx, ly as int lists."""
    rng = np.random.default_rng(seed)
    N = len(T_n)
    T = T or max(T_n)
    U1 = U1 or max(U_n) + 1
    f = (rng.standard_normal((N, T, V)) * scale).astype(np.float32)
    g = (rng.standard_normal((N, U1, V)) * scale).astype(np.float32)
    labels = rng.integers(0, V - 1, (N, max(U1 - 1, 0))).astype(np.int32) if V > 1 else np.zeros((N, U1 - 1), np.int32)
    labels = labels + (labels >= blank)                                  # every column but the blank's
    return f, g, labels.astype(np.int32), [int(t) for t in T_n], [int(u) for u in U_n]


def peaked_case(offset, seed=0):
    """The input on which a normaliser factored into a maximum of f and one of g underflows: T = 40, U1 = 21, V = 9, both inputs
    3 N(0, 1), `offset` added to column 1 of f and to column 2 of g (60 and 120 are exact in bf16)."""
    f, g, labels, lx, ly = random_case(seed, [40], [20], 9, 0)
    f[:, :, 1] += np.float32(offset)
    g[:, :, 2] += np.float32(offset)
    return f, g, labels, lx, ly
