"""cat_amd.ctc_crf -- the Python surface CAT imports from ``ctc_crf`` (reference
src/ctc_crf/ctc_crf/__init__.py), backed by the MI355X-native HIP library (cat_amd/csrc).

Same names, arguments and error behaviour as the reference:
  CTC_CRF_LOSS(lamb=0.1, size_average=True)(logits, labels, lx, ly) -> FloatTensor[1]   (:97-125)
  WARP_CTC_LOSS(size_average=True, blank_label=0, fuse_log_softmax=False, time_major=False)(logits, labels, input_lengths, label_lengths)
                                                                                         (:128-144; the keywords after size_average added)
  CRFContext(den_lm, gpus)                                                               (:147-171)
  _CTC_CRF, _WARP_CTC_GPU  autograd Functions                                             (:25-94)
  ctc_align(log_probs, labels, input_lengths, label_lengths, blank=0, time_major=False, fuse_log_softmax=False) -> (pos, tokens, scores)
                                                                                         (forced alignment; not in the reference)
  ctc_score(log_probs, hyps, hyp_lengths, input_lengths, hyp_utt=None, blank=0, time_major=False, fuse_log_softmax=False,
            max_hyp_len=None) -> FloatTensor[H]                                          (forward-only scores of many hypotheses per utterance)
  ctc_logp(log_probs, hyps, hyp_lengths, input_lengths, hyp_utt=None, blank=0, time_major=False, max_hyp_len=None, fuse_log_softmax=False)
                                                                                         -> (FloatTensor[H], IntTensor[H])
                                                                                         (the same scores WITH autograd: one [N,T,V] gradient)
                                                                                         (both: hypotheses on the CPU, or on the device as the
                                                                                         padded rows ctc_sample / ctc_beam_search return, bounded
                                                                                         by max_hyp_len -- no copy to the host, no stream drain)
  ctc_sample(log_probs, input_lengths, n_samples, seed, offset=0, blank=0, time_major=False, return_paths=False)
                                                              -> (hyps IntTensor[N*K, T], hyp_lengths IntTensor[N*K], hyp_utt IntTensor[N*K])
                                                                                         (K label sequences per utterance drawn on the GPU)
  ctc_greedy(log_probs, input_lengths, blank=0, time_major=False) -> (hyps IntTensor[N, T], hyp_lengths IntTensor[N])   (best path)
  ctc_beam_search(log_probs, input_lengths, beam_size=16, nbest=1, top_classes=40, blank=0, time_major=False, fuse_log_softmax=False,
                  return_trace=False, lm=None, alpha=0.0, beta=0.0, return_lm_scores=False)
                                       -> (hyps IntTensor[N*nbest, T], hyp_lengths IntTensor[N*nbest], hyp_utt IntTensor[N*nbest],
                                           scores FloatTensor[N*nbest])                  (prefix beam search: the N-best lists; with lm
                                                                                         shallow fusion of a token-level n-gram LM)
  ctc_beam_search_chunk(log_probs, input_lengths, state=None, reset=None, beam_size=16, nbest=1, top_classes=40, blank=0,
                        time_major=False, fuse_log_softmax=False, lm=None, alpha=0.0, beta=0.0, max_hyp_len=512, return_trace=False,
                        return_lm_scores=False) -> (BeamState, hyps IntTensor[N*nbest, max_hyp_len], hyp_lengths, hyp_utt, scores)
                                                                                         (streaming: the same search chunk by chunk, the beam
                                                                                         carried in a BeamState; any split gives the same bits)
  NgramLM.from_arpa(path, vocab_size, unk_logp=None), NgramLM.from_ngrams(dict, vocab_size, unk_logp=None)
                                                                                         (the LM of ctc_beam_search: cat_amd/ngram_lm.py)
  ctc_edit_distance(hyps, hyp_lengths, labels, label_lengths, hyp_utt=None, return_ops=False) -> dist IntTensor[H]
                                                              (with return_ops: (dist, sub, dele, ins), each IntTensor[H])
                                                                                         (token errors of hypotheses on the GPU: WER / PER sums, the MWER risk)
  ngram_score(hyps, hyp_lengths, lm, bos=True, eos=False, return_token_scores=False) -> (scores FloatTensor[H], invalid IntTensor[H])
                                                              (with return_token_scores: also token_logp [H, W], token_order [H, W])
                                                                                         (n-gram LM scores of rows on the GPU: N-best rescoring)
  rnnt_loss(log_probs, labels, frames_lengths, labels_lengths, average_frames=False, reduction=None, blank=0, compact=False,
            fuse_log_softmax=False) -> costs                                             (warp_rnnt.rnnt_loss: the RNN-T transducer loss with
                                                                                         autograd, padded or compact joiner output, normalised
                                                                                         or raw; the top-level package warp_rnnt re-exports it)
  rnnt_loss_simple(f_enc, g_pred, labels, frames_lengths, labels_lengths, average_frames=False, reduction=None, blank=0) -> costs
                                                                                         (warp_rnnt.rnnt_loss_simple: the same loss of the joiner
                                                                                         f + g from f (N, T, V) and g (N, U+1, V) alone, the
                                                                                         (N, T, U+1, V) tensor never formed; re-exported likewise)
  ctct_loss(log_probs, labels, frames_lengths, labels_lengths, average_frames=False, reduction=None, blank=0, fuse_log_softmax=False)
            -> costs                                                                     (warp_ctct.ctct_loss: the CTC-Transducer loss with
                                                                                         autograd on the padded joiner output, normalised or
                                                                                         raw; the top-level package warp_ctct re-exports it)
plus the functional form named by BASELINE.json:
  ctc_crf_loss(log_probs, labels, frame_lens, label_lens, den_lm, lamb=0.1, size_average=True)

Differences that are deliberate (DESIGN.md "boundary"): no host synchronisation in forward (the
reference has three), the loss stays on the GPU, and utterances the reference treats as
invalid (L + repeats > T) contribute 0 to the numerator instead of uninitialised memory.
"""
import os
from typing import Dict, List, Tuple, Union

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn import Module

from . import _C as core
from ._C import BeamState  # noqa: F401
from ..ngram_lm import NgramLM  # noqa: F401

__version__ = "0.1.0"


def _assert_no_grad(tensor):
    assert not tensor.requires_grad, "shouldn't require grads"


class _WARP_CTC_GPU(Function):
    """Plain CTC NLL (reference __init__.py:25-55): costs = -sum_b logp_b, grad = -gamma_ctc.
    blank_label (not in the reference's Function; warp-ctc's ctcOptions::blank_label): the blank's column.
    time_major (as torch.nn.CTCLoss): logits and the gradient are (T, N, V), read and written in place."""

    @staticmethod
    def forward(ctx, logits, labels, input_lengths, label_lengths, size_average=True, blank_label=0, time_major=False):
        logits = logits.contiguous()
        batch_size = logits.size(1 if time_major else 0)
        s = 1.0 / batch_size if size_average else 1.0
        costs, grads, _ = core.loss_fwd_bwd(logits, labels, input_lengths, label_lengths, 0.0, s, None, blank=int(blank_label),
                                            time_major=bool(time_major))
        ctx.grads = grads
        return costs

    @staticmethod
    def backward(ctx, grad_output):
        return ctx.grads * grad_output.to(ctx.grads.device), None, None, None, None, None, None


class _WARP_CTC_LOGITS_GPU(Function):
    """_WARP_CTC_GPU with the log_softmax in front of it fused in (the caller's ``torch.log_softmax(x.float(), -1)``,
    cat/ctc/train.py:191-196): takes the RAW network output in fp32 / bf16 / fp16, (N, T, V) or (T, N, V); the loss is that of
    log_softmax(netout), the gradient d loss / d netout is computed in fp32 and returned in netout's dtype (as _CTC_CRF_LOGITS)."""

    @staticmethod
    def forward(ctx, netout, labels, input_lengths, label_lengths, size_average=True, blank_label=0, time_major=False):
        netout = netout.contiguous()
        batch_size = netout.size(1 if time_major else 0)
        s = 1.0 / batch_size if size_average else 1.0
        costs, grads, _ = core.loss_fwd_bwd(netout, labels, input_lengths, label_lengths, 0.0, s, None, fused=True,
                                            blank=int(blank_label), time_major=bool(time_major))
        ctx.grads = grads
        ctx.out_dtype = netout.dtype
        return costs

    @staticmethod
    def backward(ctx, grad_output):
        return (ctx.grads * grad_output.to(ctx.grads.device)).to(ctx.out_dtype), None, None, None, None, None, None


class _CTC_CRF(Function):
    """reference __init__.py:58-94:
    costs = sum_b [logZ_den(b) - (1+lamb) logp_ctc(b)], grads = gamma_den - (1+lamb) gamma_ctc,
    both / N when size_average.  One fused native call instead of gpu_ctc + gpu_den + 5 torch ops."""

    @staticmethod
    def forward(ctx, logits, labels, input_lengths, label_lengths, lamb=0.1, size_average=True):
        logits = logits.contiguous()
        batch_size = logits.size(0)
        s = 1.0 / batch_size if size_average else 1.0
        costs, grads, _ = core.loss_fwd_bwd(logits, labels, input_lengths, label_lengths, s, s * (1.0 + lamb),
                                            core.graph_for(logits.device))
        ctx.grads = grads
        return costs

    @staticmethod
    def backward(ctx, grad_output):
        return ctx.grads * grad_output.to(ctx.grads.device), None, None, None, None, None, None


class _CTC_CRF_LOGITS(Function):
    """_CTC_CRF with the log_softmax in front of it fused in (the caller's
    ``logits = torch.log_softmax(netout, -1)`` + ``criterion(logits.float(), ...)``, cat/ctc/train.py:174-186):
    takes the RAW network output in fp32 / bf16 / fp16, the loss is that of log_softmax(netout), the gradient
    is d loss / d netout (log_softmax's backward included), computed in fp32 and returned in netout's dtype."""

    @staticmethod
    def forward(ctx, netout, labels, input_lengths, label_lengths, lamb=0.1, size_average=True):
        netout = netout.contiguous()
        batch_size = netout.size(0)
        s = 1.0 / batch_size if size_average else 1.0
        costs, grads, _ = core.loss_fwd_bwd(netout, labels, input_lengths, label_lengths, s, s * (1.0 + lamb),
                                            core.graph_for(netout.device), fused=True)
        ctx.grads = grads
        ctx.out_dtype = netout.dtype
        return costs

    @staticmethod
    def backward(ctx, grad_output):
        return (ctx.grads * grad_output.to(ctx.grads.device)).to(ctx.out_dtype), None, None, None, None, None, None


class CTC_CRF_LOSS(Module):
    def __init__(self, lamb: float = 0.1, size_average: bool = True, fuse_log_softmax: bool = False):
        """
        lamb (float): weight for auxiliary CTC loss, final loss = lamb * loss_ctc + loss_crf
        size_average (bool): whether to do average over batch size dimension.
        fuse_log_softmax (bool, not in the reference): ``forward`` takes the RAW network output (fp32, bf16 or
            fp16) instead of log-probs; log_softmax and its backward run inside the loss kernels.
        """
        super(CTC_CRF_LOSS, self).__init__()
        self.ctc_crf = _CTC_CRF_LOGITS.apply if fuse_log_softmax else _CTC_CRF.apply
        self.lamb = lamb
        self.size_average = size_average
        self.fuse_log_softmax = fuse_log_softmax

    def forward(self, logits, labels, lx, ly) -> torch.FloatTensor:
        """
        logits (torch.FloatTensor): size (N, T, V), on GPU device (log-probs; no softmax is applied).
        labels (torch.IntTensor)  : size (sum(ly), ) flattened without padding, on CPU
        lx (torch.IntTensor) : size (N, ), on CPU
        ly (torch.IntTensor) : size (N, ), on CPU
        """
        assert len(labels.size()) == 1
        if self.fuse_log_softmax:
            assert logits.dtype in (torch.float, torch.bfloat16, torch.float16), f"expect float/bfloat16/float16 network output, instead: {logits.dtype}"
        else:
            assert logits.dtype == torch.float, f"expect logits to be torch.float object, instead: {logits.dtype}"
        assert labels.dtype == torch.int, f"expect labels to be torch.int object, instead: {labels.dtype}"
        assert lx.dtype == torch.int, f"expect lx to be torch.int object, instead: {lx.dtype}"
        assert ly.dtype == torch.int, f"expect ly to be torch.int object, instead: {ly.dtype}"
        _assert_no_grad(labels)
        _assert_no_grad(lx)
        _assert_no_grad(ly)
        return self.ctc_crf(logits, labels, lx, ly, self.lamb, self.size_average)


class WARP_CTC_LOSS(Module):
    """Kept for parity with the reference (which itself recommends torch.nn.CTCLoss)."""

    def __init__(self, size_average=True, blank_label=0, fuse_log_softmax=False, time_major=False):
        """blank_label (not in the reference, which fixes 0; as torch.nn.CTCLoss(blank=...)): the blank's column of the log-probs;
        labels then lie in [0, V) without it.
        fuse_log_softmax (not in the reference): ``forward`` takes the RAW network output (fp32, bf16 or fp16) instead of log-probs;
            log_softmax and its backward run inside the loss kernels, the gradient comes back in the input's dtype.
        time_major (not in the reference): logits are (T, N, V), as torch.nn.CTCLoss takes them, read in place."""
        super(WARP_CTC_LOSS, self).__init__()
        self.ctc = _WARP_CTC_LOGITS_GPU.apply if fuse_log_softmax else _WARP_CTC_GPU.apply
        self.size_average = size_average
        self.blank_label = blank_label
        self.fuse_log_softmax = fuse_log_softmax
        self.time_major = time_major

    def forward(self, logits, labels, input_lengths, label_lengths):
        assert len(labels.size()) == 1
        _assert_no_grad(labels)
        _assert_no_grad(input_lengths)
        _assert_no_grad(label_lengths)
        if self.fuse_log_softmax:
            assert logits.dtype in (torch.float, torch.bfloat16, torch.float16), f"expect float/bfloat16/float16 network output, instead: {logits.dtype}"
        return self.ctc(logits, labels, input_lengths, label_lengths, self.size_average, self.blank_label, self.time_major)


class CRFContext:
    def __init__(self, den_lm: str, gpus: Union[int, List[int]]) -> None:
        """
        den_lm (str): path to the denominator LM (OpenFst vector/standard binary, as produced by
            cat/utils/tool/prep_den_lm.sh).
        gpus   (int, List[int]): which GPU(s) to load it on.
        """
        if not os.path.isfile(den_lm):
            raise RuntimeError(f"Denominator LM model location is invalid: {den_lm}.")
        if isinstance(gpus, int):
            gpus = [gpus]
        nprocs = torch.cuda.device_count()
        if not all([i >= 0 and i < nprocs for i in gpus]):
            raise RuntimeError(f"Available GPU={nprocs}, invalid GPU ids: {gpus}.")
        gpus_t = torch.IntTensor(gpus)
        core.init_env(den_lm, gpus_t)
        self._gpus = gpus_t
        # the graphs THIS context created: __del__ releases these and nothing else (a later context on the same
        # device replaces the graph; the reference's Release() would free whatever is current, den_calculate.cu:394-425)
        self._handles = {int(i): core.graph_generation(int(i)) for i in gpus}   # {device: generation of the graph}
        self.den_lm = den_lm

    def owns_graph(self, idx: int) -> bool:
        """True while the graph this context loaded on device `idx` is still the device's current graph."""
        gen = getattr(self, '_handles', {}).get(idx)
        return gen is not None and core.graph_generation(idx) == gen

    def __del__(self):
        if hasattr(self, '_handles'):
            try:
                core.release_handles(self._handles)
            except Exception:  # interpreter shutdown
                pass
            del self._handles


def ctc_align(log_probs: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor, label_lengths: torch.Tensor,
              blank: int = 0, time_major: bool = False, fuse_log_softmax: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Forced alignment (not in the reference): the single best CTC alignment of every transcript, on the GPU.

    log_probs (torch.FloatTensor): (N, T, V) log-probs on the GPU, or (T, N, V) with time_major=True; read in place.
    labels, input_lengths, label_lengths (torch.IntTensor): on the CPU, labels flattened without padding as for WARP_CTC_LOSS.
    blank (int): the blank's column; labels lie in [0, V) without it (in [1, V) for blank = 0).
    fuse_log_softmax (bool): log_probs is the RAW network output in fp32, bf16 or fp16 (no log_softmax, no fp32 copy): the path is the
        best one on the upcast values -- the best under log_softmax as well, since every alignment collects the same normalisers --
        and scores are the log-probabilities under log_softmax.

    Returns (pos, tokens, scores), all on log_probs' device, without a host synchronisation and without autograd:
      pos    IntTensor[N, T]: the index k in [0, label_lengths[n]) of the transcript position emitted at frame t, -1 for a blank
             frame, -2 for t >= input_lengths[n];
      tokens IntTensor[N, T]: the class emitted at frame t -- labels[k], the blank's index where pos == -1, -1 where pos == -2;
      scores FloatTensor[N] : the log-probability of the path (-inf, and a row of -2: no alignment exists -- the transcript does
             not fit into input_lengths[n] frames, or every alignment has probability 0).
    Among alignments of equal score the one that stays longest in each state wins (stay, then advance, then skip a blank)."""
    assert len(labels.size()) == 1
    if fuse_log_softmax:
        assert log_probs.dtype in (torch.float, torch.bfloat16, torch.float16), f"expect float/bfloat16/float16 network output, instead: {log_probs.dtype}"
    else:
        assert log_probs.dtype == torch.float, f"expect log_probs to be torch.float object, instead: {log_probs.dtype}"
    with torch.no_grad():
        pos, tokens, scores, _ = core.ctc_align(log_probs.detach().contiguous(), labels, input_lengths, label_lengths, int(blank),
                                                bool(time_major), fused=bool(fuse_log_softmax))
    return pos, tokens, scores


def ctc_score(log_probs: torch.Tensor, hyps: torch.Tensor, hyp_lengths: torch.Tensor, input_lengths: torch.Tensor,
              hyp_utt: torch.Tensor = None, blank: int = 0, time_major: bool = False, fuse_log_softmax: bool = False,
              max_hyp_len: int = None) -> torch.Tensor:
    """Forward-only CTC log-likelihoods of H hypotheses over N utterances (not in the reference, whose callers loop over
    nn.CTCLoss(reduction='none') under no_grad, or score N*K hypotheses on repeat_interleave'd activations: cat/ctc/train_jsa.py:147-160,
    decode_jsa_mls.py:189-191).  The activations are read in place and never replicated; there is no backward chain and no gradient.

    log_probs (torch.FloatTensor): (N, T, V) log-probs on the GPU, or (T, N, V) with time_major=True.
    hyps (torch.IntTensor): on the CPU, either flattened (sum(hyp_lengths),) or padded (H, Lmax) as nn.CTCLoss takes targets; of a padded
        row the first hyp_lengths[h] entries count.
    hyp_lengths (torch.IntTensor): (H,), on the CPU.   input_lengths (torch.IntTensor): (N,), on the CPU.
    hyp_utt (torch.IntTensor): (H,), on the CPU: the utterance in [0, N) each hypothesis is scored on, in any order; an utterance may own
        none.  None: H = N and hypothesis h is scored on utterance h -- under no_grad this is -nn.CTCLoss(reduction='none').
    blank (int): the blank's column; labels lie in [0, V) without it.
    fuse_log_softmax (bool): log_probs is the RAW network output in fp32, bf16 or fp16; the scores are those of log_softmax.

    Hypotheses that are already ON THE DEVICE -- the rows ctc_sample, ctc_greedy and ctc_beam_search return -- are scored where they lie:
    hyps is then an (H, W) int32 tensor on log_probs' device with contiguous rows, hyp_lengths and hyp_utt are (H,) int32 tensors on
        that device (hyp_utt=None: H = N, an arange built on the device), input_lengths may stay on the CPU or lie on the device.  The
        three travel together: a mix of CPU and CUDA tensors among hyps, hyp_lengths and hyp_utt is refused.  Nothing is copied to the
        host and the stream is never drained.
    max_hyp_len (int): device hypotheses only (with CPU hypotheses it must be None: the host knows the lengths there).  A bound on
        hyp_lengths that the caller promises; default min(W, 2047), a larger value is refused.  The host never reads the lengths, so a
        hypothesis over the bound (or with a negative length, a label outside [0, V) or an utterance outside [0, N)) is NOT an
        exception: it comes back with -inf.  Each hypothesis is scored by the kernel of its own length class, so its score does not
        depend on the bound or on its neighbours; a tight bound only saves the passes over the classes above it.

    Returns FloatTensor[H] on log_probs' device: +log p(hyp | utterance), -inf for a hypothesis that has no alignment (it does not fit
    into input_lengths[u] frames, or every alignment has probability 0).  No host synchronisation.  The result carries NO autograd
    history -- requires_grad is False even for an input that requires grad: this is a scoring call, not a loss.
    A hypothesis's score is the same bits wherever it stands in the list and in either layout."""
    on_device = core.device_rows("ctc_score", hyps, hyp_lengths, hyp_utt, max_hyp_len)   # (placement only: needs no device)
    if fuse_log_softmax:
        assert log_probs.dtype in (torch.float, torch.bfloat16, torch.float16), f"expect float/bfloat16/float16 network output, instead: {log_probs.dtype}"
    else:
        assert log_probs.dtype == torch.float, f"expect log_probs to be torch.float object, instead: {log_probs.dtype}"
    if not log_probs.is_cuda:
        raise RuntimeError("ctc_score: log_probs must be on the GPU (there is no CPU path)")
    with torch.no_grad():
        scores, _ = core.ctc_score(log_probs.detach().contiguous(), hyps, hyp_lengths, input_lengths, hyp_utt, int(blank), bool(time_major),
                                   fused=bool(fuse_log_softmax), max_hyp_len=max_hyp_len if on_device else None)
    return scores


class _CTC_LOGP(Function):
    """scores [H] = crf_ctc_score; backward = ONE crf_ctc_score_grad call with weight = grad_output, on the metadata forward staged."""

    @staticmethod
    def forward(ctx, log_probs, sm, time_major):
        scores, invalid = core.ctc_score_staged(log_probs, sm, time_major)
        ctx.save_for_backward(log_probs)
        ctx.sm, ctx.time_major = sm, time_major
        ctx.mark_non_differentiable(invalid)
        return scores, invalid

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_scores, _grad_invalid):
        log_probs, = ctx.saved_tensors
        w = grad_scores.to(device=log_probs.device, dtype=torch.float32).contiguous()
        grad, _, _ = core.ctc_score_grad(log_probs, ctx.sm, w, ctx.sm.blank, ctx.time_major)
        return grad, None, None


class _CTC_LOGP_LOGITS(Function):
    """_CTC_LOGP on the RAW network output in fp32 / bf16 / fp16: scores [H] = crf_ctc_score_logits; backward = ONE crf_ctc_score_grad_logits
    call with weight = grad_output, whose fp32 result -- d / d netout, log_softmax's backward included -- is cast once to netout's dtype
    (as _CTC_CRF_LOGITS).  No fp32 copy of the activations is made or kept."""

    @staticmethod
    def forward(ctx, netout, sm, time_major):
        scores, invalid = core.ctc_score_staged(netout, sm, time_major, fused=True)
        ctx.save_for_backward(netout)
        ctx.sm, ctx.time_major = sm, time_major
        ctx.mark_non_differentiable(invalid)
        return scores, invalid

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_scores, _grad_invalid):
        netout, = ctx.saved_tensors
        w = grad_scores.to(device=netout.device, dtype=torch.float32).contiguous()
        grad, _, _ = core.ctc_score_grad(netout, ctx.sm, w, ctx.sm.blank, ctx.time_major, fused=True)
        return grad.to(netout.dtype), None, None


def ctc_logp(log_probs: torch.Tensor, hyps: torch.Tensor, hyp_lengths: torch.Tensor, input_lengths: torch.Tensor,
             hyp_utt: torch.Tensor = None, blank: int = 0, time_major: bool = False, max_hyp_len: int = None,
             fuse_log_softmax: bool = False):
    """ctc_score with autograd: CTC log-likelihoods of H hypotheses over N utterances whose gradient reaches log_probs as ONE (N, T, V)
    tensor -- what minimum-risk / MWER training on sampled or N-best hypotheses and the nn.CTCLoss(reduction='none',
    zero_infinity=True) / length losses (cat/ctc/train_jsa.py:194-201) need, without repeat_interleave'd activations and without an
    (H, T, V) gradient.  MWER in three lines, the hypotheses never leaving the device:

        hyps, hyp_lengths, hyp_utt = ctc_sample(log_probs, input_lengths, K, seed)
        scores, _ = ctc_logp(log_probs, hyps, hyp_lengths, input_lengths, hyp_utt)
        (torch.softmax(scores.view(N, K), -1) * risk.view(N, K)).sum().backward()

    log_probs (torch.FloatTensor): (N, T, V) fp32 log-probs on the GPU, contiguous, or (T, N, V) with time_major=True; anything else is
        refused.  hyps, hyp_lengths, input_lengths, hyp_utt, blank: as ctc_score takes them -- CPU tensors, or device rows: (H, W) int32
        hyps with (H,) int32 hyp_lengths and hyp_utt on log_probs' device, scored and differentiated where they lie; forward and backward
        share one plan, nothing is staged twice, nothing is read on the host.
    max_hyp_len (int): device rows only (None with CPU hypotheses), the caller's bound on hyp_lengths; pass it by keyword.  Default
        min(W, 2047) for an input that does not require grad, min(W, 255) for one that does; a larger value is refused before any call.
        A hypothesis over the bound is NOT an exception -- the host never reads the lengths: it comes back with invalid = 1, a score of
        -inf and zero gradient.  The gradient's workspace, 8 bytes x H x T x (64, 128, 256 or 512 states for a bound of up to 31, 63,
        127, 255), grows with the class of max_hyp_len, NOT with the true lengths: a caller who knows a bound should pass it (sampled rows
        are W = T wide, so the default is the largest class whenever T >= 128).
    fuse_log_softmax (bool): log_probs is the RAW network output in fp32, bf16 or fp16, read in place -- no log_softmax in front, no fp32
        copy kept for autograd: the scores are ctc_score(fuse_log_softmax=True)'s bits, those of log_softmax of the upcast values, and
        backward is one call (crf_ctc_score_grad_logits) whose fp32 gradient with respect to the raw output, log_softmax's backward
        included, is cast once to the input's dtype.
    Returns (scores FloatTensor[H], invalid IntTensor[H]) on log_probs' device, no host synchronisation.  scores are ctc_score's bits and
    differentiable with respect to log_probs (once: no double backward); invalid (1: the hypothesis does not fit its utterance) is not.
    Backward is one call (include/ctc_crf_hip.h crf_ctc_score_grad) whose weights are the incoming grad_output, so any torch expression
    of the scores trains; a hypothesis that is invalid or scores -inf, or whose weight is exactly 0, adds nothing to the gradient
    (zero_infinity=True).  With log_probs.requires_grad no hypothesis may be longer than 255 labels."""
    on_device = core.device_rows("ctc_logp", hyps, hyp_lengths, hyp_utt, max_hyp_len)   # (placement only: needs no device)
    if fuse_log_softmax:
        if log_probs.dtype not in (torch.float, torch.bfloat16, torch.float16):
            raise RuntimeError(f"ctc_logp: expect float32, bfloat16 or float16 network output, got {log_probs.dtype}")
    elif log_probs.dtype != torch.float:
        raise RuntimeError(f"ctc_logp: expect float32 log-probs, got {log_probs.dtype}")
    if not log_probs.is_cuda:
        raise RuntimeError("ctc_logp: log_probs must be on the GPU (there is no CPU path)")
    if log_probs.dim() != 3 or not log_probs.is_contiguous():
        raise RuntimeError("ctc_logp: expect contiguous (N, T, V) or (T, N, V) log-probs")
    if on_device:                              # (no value of a device tensor is read here: the bound is the caller's)
        with torch.no_grad():
            sr = core.stage_score_rows(log_probs, hyps, hyp_lengths, input_lengths, hyp_utt, int(blank), bool(time_major), bool(fuse_log_softmax),
                                       max_hyp_len, grad=log_probs.requires_grad, who="ctc_logp")
        return (_CTC_LOGP_LOGITS if fuse_log_softmax else _CTC_LOGP).apply(log_probs, sr, bool(time_major))
    if log_probs.requires_grad and hyp_lengths.numel() and int(hyp_lengths.max()) > core.SCORE_GRAD_MAX_LEN:
        raise RuntimeError(f"ctc_logp: the gradient takes hypotheses of up to {core.SCORE_GRAD_MAX_LEN} labels, got {int(hyp_lengths.max())}")
    with torch.no_grad():
        sm = core.stage_score_meta(log_probs, hyps, hyp_lengths, input_lengths, hyp_utt, int(blank), bool(time_major), bool(fuse_log_softmax))
    return (_CTC_LOGP_LOGITS if fuse_log_softmax else _CTC_LOGP).apply(log_probs, sm, bool(time_major))


def ctc_sample(log_probs: torch.Tensor, input_lengths: torch.Tensor, n_samples: int, seed: int, offset: int = 0, blank: int = 0,
               time_major: bool = False, return_paths: bool = False):
    """K = n_samples label sequences per utterance drawn on the GPU: per frame K classes from softmax(log_probs), then the CTC collapse
    (repeats merged, blanks dropped) of each of the N K frame paths -- the reference's `_sample` (cat/ctc/train_jsa.py:256-269:
    torch.multinomial over N T rows, a transpose, a repeat of the lengths and the third-party ctc_align.align_) in one call.

    log_probs: (N, T, V) on the GPU, or (T, N, V) with time_major=True; fp32, bf16 or fp16, read in place.  Log-probs and raw network
        output are drawn from alike: the distribution is softmax of the row (for log-probs that is exp), so there is no fuse switch.
        Rows hold neither NaN nor +inf; a class at -inf is never drawn; a row of -inf only emits the blank.
    input_lengths (torch.IntTensor): (N,), on the CPU, none above T.
    seed, offset: Python ints in [0, 2^64) and [0, 2^32).  The draws are counter-based -- Philox4x32-10 on (seed, offset, n, t, k) -- and
        never touch torch's generator: for fixed (seed, offset) the sample of utterance n, draw k is the same bits in both layouts, in any
        batch (n is the index in the call), for any n_samples > k and across calls.  Advance offset (or seed) for fresh samples.

    Returns (hyps, hyp_lengths, hyp_utt) and, with return_paths, paths -- IntTensors on log_probs' device, no host synchronisation, no
    autograd history:
        hyps (N K, T): row h = n K + k holds the hyp_lengths[h] labels of the sequence, then the BLANK's index up to T (padded as
            pad_sequence(padding_value=blank) pads: the rows go straight into an embedding);
        hyp_utt (N K,): h // K, so that ctc_score(log_probs, hyps.cpu(), hyp_lengths.cpu(), input_lengths, hyp_utt.cpu()) scores them;
        paths (N K, T): the class drawn per frame, -1 for t >= input_lengths[n]."""
    with torch.no_grad():
        hyps, hyp_lengths, paths = core.ctc_sample(log_probs.detach().contiguous(), input_lengths, n_samples, seed, offset, int(blank),
                                                   bool(time_major), return_paths=bool(return_paths))
        hyp_utt = torch.arange(hyps.size(0), dtype=torch.int32, device=hyps.device).div_(int(n_samples), rounding_mode="floor")
    return (hyps, hyp_lengths, hyp_utt, paths) if return_paths else (hyps, hyp_lengths, hyp_utt)


def ctc_greedy(log_probs: torch.Tensor, input_lengths: torch.Tensor, blank: int = 0, time_major: bool = False):
    """Best-path CTC decoding on the GPU: the arg-max of every frame (the lowest class among equals, as torch.argmax), collapsed.

    log_probs: (N, T, V) on the GPU, or (T, N, V) with time_major=True; fp32, bf16 or fp16 log-probs or raw network output, read in place.
    input_lengths (torch.IntTensor): (N,), on the CPU, none above T.
    Returns (hyps IntTensor[N, T], hyp_lengths IntTensor[N]) on log_probs' device, hyps padded with the blank's index; no host
    synchronisation, no autograd history."""
    with torch.no_grad():
        hyps, hyp_lengths, _ = core.ctc_sample(log_probs.detach().contiguous(), input_lengths, 1, 0, 0, int(blank), bool(time_major),
                                               greedy=True)
    return hyps, hyp_lengths


def ctc_beam_search(log_probs: torch.Tensor, input_lengths: torch.Tensor, beam_size: int = 16, nbest: int = 1, top_classes: int = 40,
                    blank: int = 0, time_major: bool = False, fuse_log_softmax: bool = False, return_trace: bool = False, lm: NgramLM = None,
                    alpha: float = 0.0, beta: float = 0.0, return_lm_scores: bool = False):
    """CTC prefix beam search on the GPU: the N-best lists that ctc_score rescores and ctc_logp trains on -- what the callers get
    from the third-party CPU ctcdecode.CTCBeamDecoder(beam_width=16, num_processes=6) after copying the whole (N, T, V) tensor to the host
    (cat/ctc/train.py:273-281, train_jsa.py:467-476, decode.py:163-222), in one call without a host round trip.  With lm it is the
    decoder's other half, CTCBeamDecoder(model_path=<KenLM n-gram>, alpha=, beta=, is_token_based=True): shallow fusion of a token-level
    n-gram LM read from the ARPA file that lmplz writes (NgramLM.from_arpa; a token is a class of log_probs).  Not covered: an
    end-of-sentence term in the search (it is in ngram_score, not in the search), word-level LMs and lexicons, KenLM's binary formats,
    an LM in ctc_sample.

    log_probs: (N, T, V) on the GPU, or (T, N, V) with time_major=True; fp32, bf16 or fp16, read in place: log-probs, or with
        fuse_log_softmax=True the RAW network output (log_softmax of the upcast values inside the call).
    input_lengths (torch.IntTensor): (N,), on the CPU, none above T.
    beam_size: prefixes kept per frame, 1 .. 64.  nbest: ranks returned per utterance, 1 .. beam_size.
    top_classes: besides the blank, only this many classes of largest value take part in a frame (1 .. 64; ctcdecode's cutoff_top_n);
        with top_classes >= V - 1 nothing is pruned.  A repeat of the last label is pruned with its class, as ctcdecode does.
    Prefixes are identified by their label sequence: mass that reaches a prefix of the beam along another parent is added to it.
    lm: None (same call and same bits as before; alpha and beta must then be 0), or an NgramLM over V classes: a prefix is ranked by
        score + alpha * log P_lm(prefix) + beta * len(prefix) (natural logs; the LM starts in the state of <s> where the model has one).
        The tables are uploaded once per device and kept.  alpha = beta = 0 gives the LM-free results bit for bit.

    Returns (hyps, hyp_lengths, hyp_utt, scores), then trace with return_trace, then lm_scores with return_lm_scores -- tensors on
    log_probs' device, no host synchronisation, no autograd history:
        hyps (N nbest, T) int32: row h = n nbest + r holds the hyp_lengths[h] labels of rank r, then the BLANK's index up to T -- the rows
            ctc_sample returns: ctc_score(log_probs, hyps.cpu(), hyp_lengths.cpu(), input_lengths, hyp_utt.cpu()) rescores them;
        hyp_utt (N nbest,): h // nbest;
        scores (N nbest,) fp32: log of the prefix's probability mass within the search (with lm: plus lm_scores, the fused score),
            non-increasing in r; scores (minus lm_scores) is a lower bound of the hypothesis's ctc_score; a rank the beam does not hold
            has length 0 and score -inf;
        trace (N, T, beam_size) int32: after frame t, slot k: parent_slot + 64 (class + 1), class -1 for a stay; -1 for an empty slot
            and for t >= input_lengths[n];
        lm_scores (N nbest,) fp32: alpha * log P_lm + beta * length of the rank's hypothesis (0 for a missing rank)."""
    with torch.no_grad():
        out = core.ctc_beam_search(log_probs.detach().contiguous(), input_lengths, beam_size, nbest, top_classes, int(blank), bool(time_major),
                                   bool(fuse_log_softmax), bool(return_trace), lm, alpha, beta, bool(return_lm_scores))
        hyps, hyp_lengths, scores, trace = out[:4]
        hyp_utt = torch.arange(hyps.size(0), dtype=torch.int32, device=hyps.device).div_(int(nbest), rounding_mode="floor")
    res = (hyps, hyp_lengths, hyp_utt, scores) + ((trace,) if return_trace else ()) + ((out[4],) if return_lm_scores else ())
    return res


def ctc_beam_search_chunk(log_probs: torch.Tensor, input_lengths: torch.Tensor, state: BeamState = None, reset: torch.Tensor = None,
                          beam_size: int = 16, nbest: int = 1, top_classes: int = 40, blank: int = 0, time_major: bool = False,
                          fuse_log_softmax: bool = False, lm: NgramLM = None, alpha: float = 0.0, beta: float = 0.0, max_hyp_len: int = 512,
                          return_trace: bool = False, return_lm_scores: bool = False):
    """Streaming CTC prefix beam search: ctc_beam_search on a CHUNK of frames, the beam carried from call to call in a BeamState -- for
    encoders that run chunk by chunk (cat/ctc/decode.py --streaming: model.chunk_infer; the CUSIDE / chunked trainers
    cat/ctc/train_unified.py, train_me2e_chunk.py), whose search today waits for the last chunk.  ANY split of an utterance's frames
    into chunks gives the bits of the whole-utterance call: scores, lengths, labels, lm_scores, and the chunks' traces one after the
    other are the whole call's trace.  The loop that replaces decode.py:197-222 for --streaming:

        state = None
        for chunk, chunk_lens in encoder_chunks:                  # chunk (N, Tc, V) on the GPU, chunk_lens (N,): frames of this chunk
            state, hyps, hyp_lengths, hyp_utt, scores = ctc_crf.ctc_beam_search_chunk(chunk, chunk_lens, state, beam_size=16, lm=lm,
                                                                                      alpha=alpha, beta=beta)
            # hyps[n, :hyp_lengths[n]]: the partial hypothesis of utterance n after the frames so far, on the device

    log_probs: (N, Tc, V) on the GPU, or (Tc, N, V) with time_major=True; the CHUNK's activations, dtypes and fuse_log_softmax as for
        ctc_beam_search.
    input_lengths: (N,), how many of the chunk's frames belong to each utterance: an int tensor on the CPU (checked against [0, Tc]) or
        an int32 tensor on the GPU (used as is; values outside [0, Tc] are clamped).  With 0 an utterance's state passes through
        unchanged and its outputs repeat what the state holds, so a finished utterance may stay in the batch.
    state: None (every utterance starts from the empty prefix), or the BeamState of the previous call.  A BeamState is immutable: every
        call allocates the state it returns and never writes to the one it continues from, so two continuations of one state are
        independent (branch, rewind).  It remembers beam_size, top_classes, blank, max_hyp_len, lm, alpha and beta; continuing under
        other values is a RuntimeError that names the field.  len(state), state.index_select(idx) and state.clone() recompose a batch:
        an utterance's state is one row of state.records, an (N, record_bytes) uint8 tensor.
    reset: None or (N,) bool / int, CPU or GPU: where set, the utterance starts from the empty prefix whatever the state holds -- a
        server reuses a batch slot for the next utterance.
    max_hyp_len: labels kept per prefix, 1 .. 8192.  A longer prefix keeps searching and scoring exactly as with a larger max_hyp_len;
        only its labels beyond are not kept, and hyp_lengths > max_hyp_len is how the caller sees it (ctc_score and ctc_edit_distance
        answer such rows with -inf / -1, their convention for rows over the bound).
    beam_size, nbest, top_classes, blank, lm, alpha, beta: as for ctc_beam_search.

    Returns (state, hyps, hyp_lengths, hyp_utt, scores), then trace with return_trace, then lm_scores with return_lm_scores, as
    ctc_beam_search does AS IF every utterance ended after the frames seen so far; hyps is (N nbest, max_hyp_len), trace
    (N, Tc, beam_size) holds the chunk's rows.  Tensors on log_probs' device, no host synchronisation, no autograd history.
    Not covered: endpointing, an end-of-sentence term, emitting only the stable common prefix of the beam, beam_size or top_classes
    above 64, a state that survives a change of beam_size or LM."""
    with torch.no_grad():
        state, hyps, hyp_lengths, scores, trace, lm_scores = core.ctc_beam_search_chunk(
            log_probs.detach().contiguous(), input_lengths, state, reset, beam_size, nbest, top_classes, int(blank), bool(time_major),
            bool(fuse_log_softmax), lm, alpha, beta, max_hyp_len, bool(return_trace), bool(return_lm_scores))
        hyp_utt = torch.arange(hyps.size(0), dtype=torch.int32, device=hyps.device).div_(int(nbest), rounding_mode="floor")
    return (state, hyps, hyp_lengths, hyp_utt, scores) + ((trace,) if return_trace else ()) + ((lm_scores,) if return_lm_scores else ())


def ctc_edit_distance(hyps: torch.Tensor, hyp_lengths: torch.Tensor, labels: torch.Tensor, label_lengths: torch.Tensor,
                      hyp_utt: torch.Tensor = None, return_ops: bool = False):
    """Token edit distance (Levenshtein) of H hypotheses to the transcripts of their utterances, on the GPU: how wrong the rows are that
    ctc_sample, ctc_greedy and ctc_beam_search return -- what the evaluation inside the training loop computes with a Python loop of
    Levenshtein.distance over `.cpu().tolist()` (cat/ctc/train.py:200-210 cal_wer, train_jsa.py:371-387 cal_per), and the `risk` of
    minimum-risk / MWER training:

        hyps, hl, hu = ctc_sample(log_probs, lx, K, seed)                      # or ctc_beam_search(..., nbest=K)
        risk = ctc_edit_distance(hyps, hl, labels, label_lengths, hu).float()
        scores, _ = ctc_logp(log_probs, hyps, hl, lx, hu)
        (torch.softmax(scores.view(N, K), -1) * risk.view(N, K)).sum().backward()

    hyps (H, W) int32 on the GPU: row h holds hypothesis h in its first hyp_lengths[h] entries; what stands behind is never read.
    hyp_lengths (H,), hyp_utt (H,) int32 on the GPU: hypothesis h belongs to utterance hyp_utt[h]; None: H == N, hypothesis h to utterance h.
    labels, label_lengths (N,): the flattened transcripts and their lengths, int tensors on the CPU as every loss call here takes them;
        transcripts of up to 2047 tokens (beyond 512 tokens: W <= 8192).  Tokens are compared as integers: no vocabulary, no blank.

    Returns dist (H,) int32 on the device: insertions + deletions + substitutions of the cheapest alignment; with return_ops
    (dist, sub, dele, ins), each (H,) int32: the counts of ONE optimal alignment, fixed by the rule that among predecessors of equal
    cost the diagonal one goes before the deletion and that before the insertion, so sub + dele + ins == dist, hits = label_length -
    sub - dele, and the counts are the same bits in any batch and order.  No autograd history, no host synchronisation.  A row whose
    hyp_utt lies outside [0, N) or whose length lies outside [0, W] takes -1 in every output.
    WER of a batch: ctc_edit_distance(...).sum() / label_lengths.sum() -- two sums."""
    with torch.no_grad():
        dist, ops = core.ctc_edit_distance(hyps.detach(), hyp_lengths, labels, label_lengths, hyp_utt, bool(return_ops))
    return (dist, ops[:, 0], ops[:, 1], ops[:, 2]) if return_ops else dist


def ngram_score(hyps: torch.Tensor, hyp_lengths: torch.Tensor, lm: NgramLM, bos: bool = True, eos: bool = False,
                return_token_scores: bool = False):
    """n-gram LM scores of hypothesis rows that lie on the GPU: log P_lm of the second pass -- what cat/lm/rescore.py:168-177 gets per
    N-best entry from cat/shared/decoder.py:542-572 (NGram.score: `.cpu()`, a Python list of strings and one kenlm.Model.score call per
    sentence) and cat/utils/lm/lmweight_search.py computes again for every (alpha, beta) -- for the rows of ctc_sample, ctc_greedy and
    ctc_beam_search, with any model, independent of the weights.

    Rescoring (ac: the acoustic scores, ctc_score's or the search's; rows of one utterance adjacent):

        lm_s, _ = ngram_score(hyps, hyp_lengths, lm, eos=True)
        total = ac + alpha * lm_s + beta * hyp_lengths
        best = total.view(N, nbest).argmax(1)

    The weight grid of lmweight_search.py (alphas, betas of shape (G,); dist = ctc_edit_distance(hyps, hyp_lengths, labels, label_lengths,
    hyp_utt)): one broadcast, one gather, two sums per grid point --

        total = ac + alphas[:, None] * lm_s + betas[:, None] * hyp_lengths                 # (G, H)
        best = total.view(G, N, nbest).argmax(2)                                           # (G, N)
        wer = dist.view(N, nbest).expand(G, N, nbest).gather(2, best[..., None]).sum((1, 2)) / label_lengths.sum()

    hyps (H, W) int32 on the GPU, W <= 8192: row h holds hypothesis h in its first hyp_lengths[h] entries; what stands behind is never read.
        Rows a stride apart are taken as ctc_score takes them.
    hyp_lengths (H,) int32 on the same GPU.  CPU tensors raise ValueError: on the host NgramLM.score is the way.
    lm: an NgramLM; its tables and eos_logp are uploaded once per device and kept.  lm.vocab_size is compared with nothing: there are no
        activations here, a token outside [0, lm.vocab_size) makes its row invalid.
    bos: the walk starts in lm.start (the state of <s> where the model has one), else at the root.
    eos: add log P(</s> | the row) = lm.eos_logp[state behind the last token]; ValueError where the model has no </s> unigram.

    Returns (scores (H,) fp32 in natural log, invalid (H,) int32) and, with return_token_scores, token_logp (H, W) fp32 and token_order
    (H, W) int32: per position the value NgramLM.lookup gives along the walk, bit for bit, and the number of tokens of the n-gram found
    (kenlm's full_scores: where a hypothesis backs off), both 0 behind the length -- on hyps' device, no autograd history, no host
    synchronisation.  scores is the fp64 sum of the row's token_logp (and the end-of-sentence value) rounded once; a row's outputs are the
    same bits in any batch, order and call.  An invalid row (length outside [0, W], a token outside the vocabulary among its first
    hyp_lengths[h]) scores -inf with invalid = 1; mask a row with length -1 to keep it out of every sum."""
    with torch.no_grad():
        return core.ngram_score(hyps, hyp_lengths, lm, bool(bos), bool(eos), bool(return_token_scores))


_CTX_CACHE: Dict[Tuple[str, int], CRFContext] = {}


class _RNNT_LOSS(Function):
    """costs [N] = crf_rnnt_loss / crf_rnnt_loss_logits; backward = ONE crf_rnnt_grad / crf_rnnt_grad_logits call on the forward's workspace
    with grad_output as the per-utterance weights.  The gradient has the input's shape and dtype; the kernels write every element."""

    @staticmethod
    def forward(ctx, log_probs, labels, lx, ly, blank, compact, fused):
        costs, invalid, call = core.rnnt_loss_fwd(log_probs, labels, lx, ly, blank, compact, fused)
        ctx.call = call
        ctx.mark_non_differentiable(invalid)
        return costs, invalid

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_costs, _grad_invalid):
        return core.rnnt_loss_bwd(ctx.call, grad_costs), None, None, None, None, None, None


def rnnt_loss(log_probs: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor, labels_lengths: torch.Tensor,
              average_frames: bool = False, reduction: str = None, blank: int = 0, compact: bool = False, fuse_log_softmax: bool = False,
              return_invalid: bool = False):
    """The RNN-T transducer loss with autograd, with the arguments and semantics of ``warp_rnnt.rnnt_loss`` (cat/rnnt/train.py:217,
    train_unified.py:292-306 call it as rnnt_loss(joinout, y, lsub, ly, compact=...)): costs[n] = -log p(y_n | x_n), summed over all
    monotone alignments -- blank moves t -> t + 1, label y[u] moves u -> u + 1, the path ends with a blank at (T_n - 1, U_n).

    log_probs: (N, T, U+1, V) float32 log-probabilities on the GPU.  Its gradient is zero except at the blank's column and at column
        labels[n, u] of every live node (t < T_n, u <= U_n).
    labels: int32 (N, U).  frames_lengths, labels_lengths: int32 (N,), both on the CPU (checked up front: ValueError) or both on the GPU
        (nothing is read on the host and nothing synchronises; an utterance out of range is invalid, see below).
    average_frames: each utterance's cost is divided by its T_n.  reduction: None / "none" (costs (N,)), "mean", "sum".
    blank: the blank's column, any of [0, V).
    compact: log_probs is (sum_n T_n (U_n + 1), V), the utterances back to back, each T_n x (U_n + 1) row-major -- what cat/rnnt/joiner.py
        produces -- and labels (sum_n U_n,), what train.py:182 makes of y.  The offsets are prefix sums taken on the device.
    fuse_log_softmax: log_probs is the RAW joiner output in float32, bfloat16 or float16, read in place: no log_softmax in front and no
        float32 copy for autograd.  The gradient comes back in the input's dtype with log_softmax's backward folded in,
        g_v - softmax_v (g_blank + g_label).
    Invalid utterances (T_n outside [1, T], U_n outside [0, U], a label outside [0, V) or equal to blank) are decided on the device: cost
    +inf and a zero gradient, as for ctc_score's rows over their bound; return_invalid=True returns (costs, invalid IntTensor[N]).  A
    lattice without a finite path (-inf entries) also costs +inf with a zero gradient, never NaN.  U <= 1023, V <= 8192.
    Not covered: gather=True as a separate mode (the kernels read two columns of a normalised row anyway), fastemit_lambda, any RNN-T
    decoding.  A joiner that is a plain sum f + g has rnnt_loss_simple below, which never forms the (N, T, U+1, V) tensor."""
    if reduction not in (None, "none", "mean", "sum"):
        raise ValueError(f"rnnt_loss: unknown reduction {reduction!r} (None, 'none', 'mean' or 'sum')")
    costs, invalid = _RNNT_LOSS.apply(log_probs, labels, frames_lengths, labels_lengths, int(blank), bool(compact), bool(fuse_log_softmax))
    if average_frames:
        costs = costs / frames_lengths.to(device=costs.device, dtype=costs.dtype)
    if reduction == "sum":
        costs = costs.sum()
    elif reduction == "mean":
        costs = costs.mean()
    return (costs, invalid) if return_invalid else costs


class _RNNT_LOSS_SIMPLE(Function):
    """costs [N] = crf_rnnt_simple_loss; backward = ONE crf_rnnt_simple_grad call on the forward's workspace with grad_output as the
    per-utterance weights.  Each gradient has its input's shape and dtype and is formed only where needs_input_grad asks; the kernels write
    every element."""

    @staticmethod
    def forward(ctx, f_enc, g_pred, labels, lx, ly, blank):
        costs, invalid, call = core.rnnt_simple_fwd(f_enc, g_pred, labels, lx, ly, blank)
        ctx.call = call
        ctx.mark_non_differentiable(invalid)
        return costs, invalid

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_costs, _grad_invalid):
        want_f, want_g = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gf, gg = core.rnnt_simple_bwd(ctx.call, grad_costs, want_f, want_g) if want_f or want_g else (None, None)
        return gf, gg, None, None, None, None


def rnnt_loss_simple(f_enc: torch.Tensor, g_pred: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor,
                     labels_lengths: torch.Tensor, average_frames: bool = False, reduction: str = None, blank: int = 0,
                     return_invalid: bool = False):
    """The RNN-T transducer loss of a joiner that is a plain sum, with autograd, with the arguments of ``warp_rnnt.rnnt_loss_simple``
    (cat/rnnt/train.py:206-213 calls it as rnnt_loss_simple(enc_out, pred_out, y, lsub, ly) for every model whose joiner is
    joiner_zoo.LogAdd, cat/rnnt/joiner.py:231-232):

        rnnt_loss_simple(f, g, labels, lf, ll, ...) == rnnt_loss((f.unsqueeze(2) + g.unsqueeze(1)).log_softmax(-1), labels, lf, ll, ...)

    computed from f and g alone: the (N, T, U+1, V) tensor is never formed, nothing of that size is allocated, and the gradients are those
    of the expression above with respect to f and g.

    f_enc (N, T, V), g_pred (N, U+1, V): raw, unnormalised, contiguous, of one dtype among float32, bfloat16 and float16, on the GPU, read
        in place; f + g is formed in float32 from their exact values.  Each gradient comes back in the input's dtype, every element
        written by the kernels (zeros for t >= T_n and u > U_n), and only where autograd asks for it.
    labels: int32 (N, U).  frames_lengths, labels_lengths: int32 (N,), both on the CPU (checked up front: ValueError) or both on the GPU
        (nothing is read on the host and nothing synchronises).  average_frames, reduction, blank, return_invalid, invalid utterances
        (cost +inf, zero gradient, invalid = 1) and lattices without a finite path (+inf, zero gradient, never NaN): as for rnnt_loss.
    Mismatched dtypes, vocabulary sizes or batch sizes and non-contiguous inputs raise ValueError.  U <= 1023, V <= 8192.
    The same bits run to run, and for an utterance alone or anywhere in a batch."""
    if reduction not in (None, "none", "mean", "sum"):
        raise ValueError(f"rnnt_loss_simple: unknown reduction {reduction!r} (None, 'none', 'mean' or 'sum')")
    costs, invalid = _RNNT_LOSS_SIMPLE.apply(f_enc, g_pred, labels, frames_lengths, labels_lengths, int(blank))
    if average_frames:
        costs = costs / frames_lengths.to(device=costs.device, dtype=costs.dtype)
    if reduction == "sum":
        costs = costs.sum()
    elif reduction == "mean":
        costs = costs.mean()
    return (costs, invalid) if return_invalid else costs


class _CTCT_LOSS(Function):
    """costs [N] = crf_ctct_loss / crf_ctct_loss_logits; backward = ONE crf_ctct_grad / crf_ctct_grad_logits call on the forward's workspace
    with grad_output as the per-utterance weights.  The gradient has the input's shape and dtype; the kernels write every element."""

    @staticmethod
    def forward(ctx, log_probs, labels, lx, ly, blank, fused):
        costs, invalid, call = core.ctct_loss_fwd(log_probs, labels, lx, ly, blank, fused)
        ctx.call = call
        ctx.mark_non_differentiable(invalid)
        return costs, invalid

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_costs, _grad_invalid):
        return core.ctct_loss_bwd(ctx.call, grad_costs), None, None, None, None, None


def ctct_loss(log_probs: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor, labels_lengths: torch.Tensor,
              average_frames: bool = False, reduction: str = None, blank: int = 0, fuse_log_softmax: bool = False,
              return_invalid: bool = False):
    """The CTC-Transducer (CTC-T) loss with autograd: what cat/rnnt/train.py:216-219 calls as ``warp_ctct.ctct_loss(xys, y, lsub, ly)`` for
    topo="ctct".  The four positional arguments are that call's; warp_ctct's source is not available, so the keywords are those of
    ``rnnt_loss`` here, not necessarily warp_ctct's own.

    A path labels EVERY frame t < T_n with one class; blanks and repeats collapse as in CTC and the collapse is the label sequence; frame
    t's emission is read from row u = the number of labels emitted before frame t.  costs[n] = -log of the sum over those paths: with
    b(t,u) = lp[t][u][blank], r(t,u) = lp[t][u][y_u] (u >= 1), e(t,u) = lp[t][u][y_{u+1}] (u < U) and the masses Ab / An after t frames with
    u labels emitted, ending in a blank (or nothing yet) / in y_u,

        Ab[0][0] = 0, everything else -inf
        Ab[t+1][u] = lse(Ab[t][u], An[t][u]) + b(t,u)
        An[t+1][u] = lse(An[t][u] + r(t,u), Ab[t][u-1] + e(t,u-1), An[t][u-1] + e(t,u-1) only if y_u != y_{u-1})
        cost = -lse(Ab[T][U], An[T][U])

    (the frame-synchronous search of cat/rnnt/ctct_decoder.py read as a sum).  With log_probs independent of u this is plain CTC.

    log_probs: (N, T, U+1, V) float32 log-probabilities on the GPU, contiguous -- the padded layout only.  Its gradient is zero except at
        the blank's column, column y_u and column y_{u+1} of every live node (t < T_n, u <= U_n); where y_u == y_{u+1} the two share a
        column and their terms add.  Over the rows u of one frame the gradient sums to -1 (times the utterance's weight).
    labels: int32 (N, U), contiguous.  frames_lengths, labels_lengths: int32 (N,), both on the CPU (checked up front) or both on the GPU
        (nothing is read on the host and nothing synchronises; an utterance out of range is invalid, see below).
    average_frames: each utterance's cost is divided by its T_n.  reduction: None / "none" (costs (N,)), "mean", "sum".
    blank: the blank's column, any of [0, V).
    fuse_log_softmax: log_probs is the RAW joiner output in float32, bfloat16 or float16, read in place; the gradient comes back in the
        input's dtype with log_softmax's backward folded in, g_v - softmax_v (g_b + g_r + g_e).
    Shapes, dtypes, non-contiguous inputs and CPU lengths out of range raise ValueError before any device call.  Invalid utterances (T_n
    outside [1, T], U_n outside [0, U], a label outside [0, V) or equal to blank) are decided on the device: cost +inf and a zero gradient;
    return_invalid=True returns (costs, invalid IntTensor[N]).  A lattice without a path -- T_n < U_n + #{u: y_u == y_{u+1}}, or -inf
    entries -- also costs +inf with a zero gradient, never NaN.  U <= 1023, V <= 8192.  The same bits run to run and for an utterance alone
    or anywhere in a batch.
    Not covered: a compact layout, the form on f and g without the joint tensor (warp_ctct.ctct_simple_loss), any CTC-T or RNN-T decoding."""
    if reduction not in (None, "none", "mean", "sum"):
        raise ValueError(f"ctct_loss: unknown reduction {reduction!r} (None, 'none', 'mean' or 'sum')")
    costs, invalid = _CTCT_LOSS.apply(log_probs, labels, frames_lengths, labels_lengths, int(blank), bool(fuse_log_softmax))
    if average_frames:
        costs = costs / frames_lengths.to(device=costs.device, dtype=costs.dtype)
    if reduction == "sum":
        costs = costs.sum()
    elif reduction == "mean":
        costs = costs.mean()
    return (costs, invalid) if return_invalid else costs


def ctc_crf_loss(log_probs: torch.Tensor, labels: torch.Tensor, frame_lens: torch.Tensor,
                 label_lens: torch.Tensor, den_lm: str, lamb: float = 0.1, size_average: bool = True,
                 fuse_log_softmax: bool = False) -> torch.Tensor:
    """Functional CTC-CRF loss (BASELINE.json north_star signature).  Lazily builds and caches the
    CRFContext for (den_lm, device) exactly as AMTrainer does (cat/ctc/train.py:180-182).
    fuse_log_softmax=True: ``log_probs`` is the raw network output (fp32 / bf16 / fp16), see _CTC_CRF_LOGITS."""
    dev = log_probs.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (os.path.abspath(den_lm), idx)
    ctx = _CTX_CACHE.get(key)
    if ctx is None or not ctx.owns_graph(idx):   # not loaded yet, or somebody replaced / released the device's graph
        ctx = None                                # (drop every reference BEFORE the replacement is created)
        for k in [k for k in _CTX_CACHE if k[1] == idx]:  # one graph per device, like the reference
            del _CTX_CACHE[k]
        _CTX_CACHE[key] = CRFContext(den_lm, idx)
    if fuse_log_softmax:
        return _CTC_CRF_LOGITS.apply(log_probs, labels.int().cpu(), frame_lens.int().cpu(), label_lens.int().cpu(),
                                     lamb, size_average)
    return _CTC_CRF.apply(log_probs.float(), labels.int().cpu(), frame_lens.int().cpu(), label_lens.int().cpu(),
                          lamb, size_average)
