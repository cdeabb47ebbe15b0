/*
 * include/ctc.h -- the warp-ctc C API, as exported by libctc_crf_hip.so (gfx950).
 *
 * The interface is that of the modified warp-ctc the reference's numerator links against
 * (gpu_ctc/ctc.h:76-109), so a binding written against it (the reference's binding.cpp gpu_ctc,
 * other warp-ctc bindings) builds and links unchanged; only the stream type is HIP's.  The work is
 * done by crf_ctc_fwd_bwd (include/ctc_crf_hip.h) on the time-major activations in place.
 *
 * Semantics
 *   - activations: device log-probabilities, time-major [maxT][minibatch][alphabet_size] float32,
 *     maxT = max(input_lengths); gradients: device memory in the same layout, or NULL for costs only.
 *   - flat_labels, label_lengths, input_lengths: HOST memory.  Labels lie in [0, alphabet_size) and
 *     differ from options.blank_label.  They are copied into the head of `workspace` on options.stream.
 *   - costs: HOST memory, one float per utterance receiving +log p(labels | activations), the modified
 *     warp-ctc's convention.  The call synchronises options.stream before it returns.
 *   - gradients receive +gamma (the per-frame label posteriors), as the reference's kernel writes them;
 *     rows t >= input_lengths[b] are zero.
 *   - an utterance without an alignment (label length + repeats > input length) gets cost 0 and zero
 *     gradient rows (warp-ctc leaves both untouched).
 *   - an utterance whose every alignment meets a -inf activation (probability 0) gets cost -inf, the
 *     exact log-probability, and zero gradient rows.
 *   - alphabet_size <= 8192 and label lengths <= 2047; larger ones are refused with
 *     CTC_STATUS_INVALID_VALUE, by get_workspace_size as by compute_ctc_loss.
 *   - workspace: device memory of get_workspace_size() bytes, for this call only.
 * Details of a failure: crf_last_error() (include/ctc_crf_hip.h).
 */
#ifndef CTC_CRF_HIP_CTC_H_
#define CTC_CRF_HIP_CTC_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef HIP_INCLUDE_HIP_HIP_RUNTIME_API_H
typedef struct ihipStream_t *hipStream_t; /* as hip_runtime_api.h declares it */
#endif

typedef enum {
    CTC_STATUS_SUCCESS = 0,
    CTC_STATUS_MEMOPS_FAILED = 1,     /* a copy to or from the device, or the stream sync, failed  */
    CTC_STATUS_INVALID_VALUE = 2,     /* a bad argument                                         */
    CTC_STATUS_EXECUTION_FAILED = 3,  /* a kernel launch failed                                 */
    CTC_STATUS_UNKNOWN_ERROR = 4
} ctcStatus_t;

/* A static, non-empty description of `status`. */
const char *ctcGetStatusString(ctcStatus_t status);

/* Zero-initialise before use (memset, or `ctcOptions o{};` in C++). */
struct ctcOptions {
    hipStream_t stream; /* all work of the call is enqueued here                  */
    int blank_label;    /* column of the blank in [0, alphabet_size)              */
};

ctcStatus_t compute_ctc_loss(const float *const activations,
                             float *gradients,
                             const int *const flat_labels,
                             const int *const label_lengths,
                             const int *const input_lengths,
                             int alphabet_size,
                             int minibatch,
                             float *costs,
                             void *workspace,
                             struct ctcOptions options);

/* Bytes of device workspace compute_ctc_loss needs for these lengths (host-only: no HIP call).
 * The size covers a gradient buffer for calls with gradients == NULL. */
ctcStatus_t get_workspace_size(const int *const label_lengths,
                               const int *const input_lengths,
                               int alphabet_size, int minibatch,
                               struct ctcOptions info,
                               size_t *size_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CTC_CRF_HIP_CTC_H_ */
