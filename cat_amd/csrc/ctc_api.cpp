// cat_amd/csrc/ctc_api.cpp -- the warp-ctc C API (include/ctc.h) on top of crf_ctc_fwd_bwd: host-resident metadata are checked
// and copied into the head of the caller's workspace, the numerator runs on the time-major activations in place, and the costs
// come back to host memory behind one stream sync (the reference's semantics, gpu_ctc.h:364-369).
// Everything this file calls inside the library is either a static helper or a crf_* symbol: a process that also loads another
// warp-ctc (the reference's own library, say) cannot redirect a call made in here to its compute_ctc_loss / get_workspace_size.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ctc.h"
#include "../../include/ctc_crf_hip.h"
#include "crf_internal.h"

namespace {

constexpr int kMaxLabelLen = crf::kMaxCtcLabelLen;   // 2L + 1 states per utterance <= the chains' 8 x 512 (crf_device.h kCtcRegs x kCtcThreads)
constexpr int kMaxAlphabet = crf::kMaxVocab;        // the limit crf_ctc_fwd_bwd applies (loss_impl)

// alphabet_size in [1, kMaxAlphabet] and minibatch > 0: checked first, before anything touches the device
ctcStatus_t check_sizes(const char *fn, int alphabet_size, int minibatch) {
    if (alphabet_size <= 0 || minibatch <= 0) {
        crf::set_error(std::string(fn) + ": alphabet_size <= 0 or minibatch <= 0");
        return CTC_STATUS_INVALID_VALUE;
    }
    if (alphabet_size > kMaxAlphabet) {
        crf::set_error(std::string(fn) + ": alphabet_size " + std::to_string(alphabet_size) + " > " + std::to_string(kMaxAlphabet) +
                       " not supported by this build");
        return CTC_STATUS_INVALID_VALUE;
    }
    return CTC_STATUS_SUCCESS;
}

int64_t al256(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct Lengths {
    int64_t maxT = 0, maxL = 0, totL = 0;
};

// the lengths of one call: INVALID_VALUE for a negative length or a label sequence longer than this build takes
ctcStatus_t scan_lengths(const int *label_lengths, const int *input_lengths, int minibatch, Lengths *out) {
    Lengths s;
    for (int b = 0; b < minibatch; ++b) {
        const int L = label_lengths[b], T = input_lengths[b];
        if (L < 0 || T < 0) { crf::set_error("negative label or input length at utterance " + std::to_string(b)); return CTC_STATUS_INVALID_VALUE; }
        if (L > kMaxLabelLen) {
            crf::set_error("label length " + std::to_string(L) + " > " + std::to_string(kMaxLabelLen) + " not supported by this build");
            return CTC_STATUS_INVALID_VALUE;
        }
        s.maxT = std::max<int64_t>(s.maxT, T);
        s.maxL = std::max<int64_t>(s.maxL, L);
        s.totL += L;
    }
    *out = s;
    return CTC_STATUS_SUCCESS;
}

// workspace of compute_ctc_loss: int32 metadata [lx | ly | label offsets | labels], the outputs [loss | costs], invalid flags,
// a gradient buffer for calls without gradients, then crf_ctc_fwd_bwd's own workspace
struct Layout {
    int64_t off_meta, off_out, off_inv, off_grad, off_crf, crf_bytes, total;
};

Layout layout(int64_t B, int64_t V, const Lengths &s) {
    Layout w{};
    int64_t o = 0;
    w.off_meta = o; o = al256(o + (3 * B + std::max<int64_t>(s.totL, 1)) * 4);
    w.off_out = o; o = al256(o + (1 + B) * 4);
    w.off_inv = o; o = al256(o + B * 4);
    w.off_grad = o; o = al256(o + s.maxT * B * V * 4);
    w.off_crf = o;
    w.crf_bytes = crf_workspace_bytes(nullptr, B, std::max<int64_t>(s.maxT, 1), V, s.maxL);
    w.total = al256(o + w.crf_bytes);
    return w;
}

ctcStatus_t from_crf(int rc) {
    if (rc == CRF_OK) return CTC_STATUS_SUCCESS;
    return rc == CRF_ERR_HIP ? CTC_STATUS_EXECUTION_FAILED : CTC_STATUS_INVALID_VALUE;
}

}  // namespace

extern "C" {

const char *ctcGetStatusString(ctcStatus_t status) {
    switch (status) {
        case CTC_STATUS_SUCCESS: return "no error";
        case CTC_STATUS_MEMOPS_FAILED: return "a device memory copy or the stream synchronisation failed";
        case CTC_STATUS_INVALID_VALUE: return "invalid value";
        case CTC_STATUS_EXECUTION_FAILED: return "kernel launch failed";
        default: return "unknown error";
    }
}

ctcStatus_t get_workspace_size(const int *const label_lengths, const int *const input_lengths, int alphabet_size, int minibatch,
                               struct ctcOptions info, size_t *size_bytes) {
    (void)info;
    if (!label_lengths || !input_lengths || !size_bytes) {
        crf::set_error("get_workspace_size: null pointer");
        return CTC_STATUS_INVALID_VALUE;
    }
    ctcStatus_t st = check_sizes("get_workspace_size", alphabet_size, minibatch);
    if (st != CTC_STATUS_SUCCESS) return st;
    Lengths s;
    st = scan_lengths(label_lengths, input_lengths, minibatch, &s);
    if (st != CTC_STATUS_SUCCESS) return st;
    *size_bytes = (size_t)layout(minibatch, alphabet_size, s).total;
    return CTC_STATUS_SUCCESS;
}

ctcStatus_t compute_ctc_loss(const float *const activations, float *gradients, const int *const flat_labels, const int *const label_lengths,
                             const int *const input_lengths, int alphabet_size, int minibatch, float *costs, void *workspace,
                             struct ctcOptions options) {
    if (!activations || !flat_labels || !label_lengths || !input_lengths || !costs || !workspace) {
        crf::set_error("compute_ctc_loss: null pointer");
        return CTC_STATUS_INVALID_VALUE;
    }
    ctcStatus_t st = check_sizes("compute_ctc_loss", alphabet_size, minibatch);
    if (st != CTC_STATUS_SUCCESS) return st;
    const int B = minibatch, V = alphabet_size, blank = options.blank_label;
    if (blank < 0 || blank >= V) {
        crf::set_error("compute_ctc_loss: blank_label " + std::to_string(blank) + " outside [0, alphabet_size=" + std::to_string(V) + ")");
        return CTC_STATUS_INVALID_VALUE;
    }
    Lengths s;
    st = scan_lengths(label_lengths, input_lengths, B, &s);
    if (st != CTC_STATUS_SUCCESS) return st;
    // metadata as crf_ctc_fwd_bwd reads it; labels in [0, V) and not the blank (the kernels index the activation rows with them)
    std::vector<int32_t> meta(3 * (size_t)B + std::max<int64_t>(s.totL, 1), 0);
    int32_t *lx = meta.data(), *ly = lx + B, *off = ly + B, *lab = off + B;
    for (int b = 0, o = 0; b < B; o += label_lengths[b], ++b) { lx[b] = input_lengths[b]; ly[b] = label_lengths[b]; off[b] = o; }
    for (int64_t i = 0; i < s.totL; ++i) {
        const int l = flat_labels[i];
        if (l < 0 || l >= V || l == blank) {
            crf::set_error("compute_ctc_loss: label " + std::to_string(l) + " at position " + std::to_string(i) + " outside [0, " + std::to_string(V) +
                           ") or equal to the blank " + std::to_string(blank));
            return CTC_STATUS_INVALID_VALUE;
        }
        lab[i] = l;
    }
    if (s.maxT == 0) {   // no frames at all: nothing to launch (every utterance has cost 0, the gradient has no rows)
        std::fill(costs, costs + B, 0.f);
        return CTC_STATUS_SUCCESS;
    }
    const Layout w = layout(B, V, s);
    char *ws = (char *)workspace;
    const hipStream_t stream = options.stream;
    int32_t *meta_d = (int32_t *)(ws + w.off_meta);
    float *out_d = (float *)(ws + w.off_out);
    if (hipMemcpyAsync(meta_d, meta.data(), meta.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess) {
        crf::set_error(std::string("compute_ctc_loss: copy of the metadata: ") + hipGetErrorString(hipGetLastError()));
        return CTC_STATUS_MEMOPS_FAILED;
    }
    // c_ctc = -1: grad = +gamma_ctc, what the reference's kernel writes (gpu_ctc_kernels.h:431-435)
    const int rc = crf_ctc_fwd_bwd(activations, 1, blank, meta_d + 3 * B, meta_d + 2 * B, meta_d, meta_d + B, B, s.maxT, V, s.maxL, -1.f,
                                   gradients ? gradients : (float *)(ws + w.off_grad), out_d, out_d + 1, (int32_t *)(ws + w.off_inv),
                                   ws + w.off_crf, w.crf_bytes, (void *)stream);
    if (rc != CRF_OK) {
        (void)hipStreamSynchronize(stream);   // (the metadata copy reads `meta`, which goes out of scope here)
        return from_crf(rc);
    }
    hipError_t e = hipMemcpyAsync(costs, out_d + 1, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, stream);
    const hipError_t e2 = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) { crf::set_error(std::string("compute_ctc_loss: copy of the costs: ") + hipGetErrorString(e)); return CTC_STATUS_MEMOPS_FAILED; }
    return CTC_STATUS_SUCCESS;
}

}  // extern "C"
