"""``import warp_ctct`` drop-in: CAT does ``import warp_ctct`` (cat/rnnt/train.py:25) and calls ``warp_ctct.ctct_loss(xys, y, lsub, ly)`` for
topo="ctct" (train.py:216-219).  With this repository's root on PYTHONPATH that import resolves to the MI355X-native implementation,
``ctc_crf.ctct_loss`` (cat_amd/ctc_crf: crf_ctct_loss / crf_ctct_grad of include/ctc_crf_hip.h), on the materialised joint tensor
(N, T, U+1, V).  ``ctct_simple_loss``, the form on f and g without that tensor, is not provided."""
from cat_amd.ctc_crf import ctct_loss  # noqa: F401


def ctct_simple_loss(*args, **kwargs):
    raise NotImplementedError("warp_ctct.ctct_simple_loss is not provided: form the joint tensor (N, T, U+1, V) and call ctct_loss on it "
                              "(fuse_log_softmax=True reads the raw joiner output in place)")
