"""``import warp_rnnt`` drop-in: CAT does ``import warp_rnnt`` (cat/rnnt/train.py:22) and ``from warp_rnnt import rnnt_loss``
(cat/rnnt/train_unified.py:26).  With this repository's root on PYTHONPATH those imports resolve to the MI355X-native implementation,
``ctc_crf.rnnt_loss`` (cat_amd/ctc_crf: crf_rnnt_loss / crf_rnnt_grad of include/ctc_crf_hip.h) and, for the models whose joiner is a plain
sum (train.py:206-213), ``ctc_crf.rnnt_loss_simple`` (crf_rnnt_simple_loss / crf_rnnt_simple_grad).  gather=True and fastemit_lambda are
not provided."""
from cat_amd.ctc_crf import rnnt_loss, rnnt_loss_simple  # noqa: F401
