// cat_amd/csrc/crf_host_util.h -- what the host units share (crf_host.hip: the loss call; crf_host_ctc.hip: forced alignment, hypothesis
// scores, sampling): the records and the rule of a workspace section, the fields inside one, the one kernel launch with its dynamic-LDS
// mark, and the choice of the numerator kernels' states per thread.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <type_traits>

#include "../../include/ctc_crf_hip.h"
#include "crf_internal.h"
#include "crf_device.h"

namespace crf {

// A workspace is a list of sections: every one starts at the running end of the layout, which then moves past its bytes to the next
// multiple of 256 (+ the ws_gap bytes).
struct WsSection { const char *name; int64_t off, bytes; };
static int64_t al(int64_t x) { return (x + 255) & ~(int64_t)255; }
// bytes no kernel may touch behind every section: the switch ws_gap x 256 (tests/guard.py); unset, the sections are packed
static int64_t ws_gap_bytes() { return 256 * (int64_t)std::max(0, opt(kOpt_ws_gap, 0)); }
// the section records as the debug exports hand them out: (offset, bytes) pairs, and the names joined by commas
static int copy_sections(const WsSection *sec, int n, int64_t *out, int n_out) {
    for (int k = 0; k < n && out && 2 * k + 1 < n_out; ++k) { out[2 * k] = sec[k].off; out[2 * k + 1] = sec[k].bytes; }
    return n;
}
static std::string join_names(const char *const *names, int n) {
    std::string s;
    for (int k = 0; k < n; ++k) { if (k) s += ','; s += names[k]; }
    return s;
}

// The arrays INSIDE a section, packed in list order: field k holds a * n + c elements of `elem` bytes (n: B, or Bp for the utterance-minor
// kernels' section) and starts where field k - 1 ends.  Entries named spare* belong to no kernel.
struct WsField { const char *name; int elem, a, c; };
// bytes in front of field k of the list (k = the number of fields: the bytes of the whole list)
static int64_t fields_off(const WsField *f, int k, int64_t n) {
    int64_t o = 0;
    for (int i = 0; i < k; ++i) o += f[i].elem * (f[i].a * n + f[i].c);
    return o;
}

// f(NR, k): states per thread (per = kCtcThreads) or lane (per = 64) as a compile-time constant, the smallest of 1, 2, 4, 8 that holds
// `states` of them, and its index k in that list
template <typename F>
static int with_nr(int64_t states, int per, F &&f) {
    const int64_t ni = (states + per - 1) / per;
    if (ni <= 1) return f(std::integral_constant<int, 1>{}, 0);
    if (ni <= 2) return f(std::integral_constant<int, 2>{}, 1);
    if (ni <= 4) return f(std::integral_constant<int, 4>{}, 2);
    return f(std::integral_constant<int, kCtcRegs>{}, 3);
}

constexpr int kMaxDev = 64;
// Dynamic LDS above 64 KiB must be opted into per kernel AND per device (hipFuncSetAttribute acts on the current
// device's copy of the function): high-water mark per device.
struct LdsMark { std::atomic<size_t> v[kMaxDev]; };
static int ensure_lds(const void *fn, size_t bytes, LdsMark &m, const char *what) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) { set_error("hipGetDevice failed"); return CRF_ERR_HIP; }
    if (bytes <= m.v[dev].load()) return CRF_OK;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) { set_error(std::string("hipFuncSetAttribute(") + what + "): " + hipGetErrorString(e)); return CRF_ERR_HIP; }
    m.v[dev] = bytes;
    return CRF_OK;
}
// Every kernel launch of the host units.  K is a template argument, so each instantiation has its own mark; a launch with dynamic LDS raises
// it first; a launch error comes back as CRF_ERR_HIP with the kernel's name (the text is built on failure only).
template <auto K, typename... A>
static int launch(const char *name, dim3 grid, dim3 block, size_t lds, hipStream_t st, const A &...args) {
    static LdsMark mark;
    int rc;
    if (lds > 0 && (rc = ensure_lds((const void *)K, lds, mark, name))) return rc;
    hipLaunchKernelGGL(K, grid, block, lds, st, args...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(std::string(name) + ": " + hipGetErrorString(e)); return CRF_ERR_HIP; }
    return CRF_OK;
}

}  // namespace crf
