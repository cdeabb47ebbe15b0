// cat_amd/csrc/crf_opts.cpp -- the library's process-wide odds and ends: the thread-local error string behind crf_last_error(),
// the registry of the run-time debug / experiment switches (crf_internal.h: CRF_OPTS) behind crf_debug_set / _unset / _list, and crf_version().
//
// Replaces the reference's error handling -- print and exit (den_calculate.cu:16-25 CHECK_CUDA, :332-333) -- by status codes with a message
// to fetch; the reference has no run-time switches.
#include <atomic>
#include <cstring>

#include "../../include/ctc_crf_hip.h"
#include "crf_internal.h"

namespace crf {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

// debug / experiment switches (crf_internal.h: CRF_OPTS)
static std::atomic<int> g_opt[kOptCount];
static std::atomic<unsigned long long> g_opt_set{0};   // bit k: switch k has a value
static_assert(kOptCount <= 64, "one bit per switch");
static const char *const kOptName[kOptCount] = {
#define CRF_OPT_NAME(name, doc) #name,
    CRF_OPTS(CRF_OPT_NAME)
#undef CRF_OPT_NAME
};
static const char *const kOptDoc[kOptCount] = {
#define CRF_OPT_DOC(name, doc) doc,
    CRF_OPTS(CRF_OPT_DOC)
#undef CRF_OPT_DOC
};
int opt(Opt k, int dflt) { return (g_opt_set.load(std::memory_order_relaxed) >> (int)k & 1ull) ? g_opt[k].load(std::memory_order_relaxed) : dflt; }
int opt_set(const char *key, int value, bool unset) {
    if (!key) { set_error("crf_debug_set: null key"); return CRF_ERR_ARG; }
    for (int k = 0; k < kOptCount; ++k)
        if (!strcmp(key, kOptName[k])) {
            if (unset) g_opt_set.fetch_and(~(1ull << k));
            else { g_opt[k].store(value); g_opt_set.fetch_or(1ull << k); }
            return CRF_OK;
        }
    set_error(std::string("crf_debug_set: unknown switch '") + key + "'");
    return CRF_ERR_ARG;
}
const char *opt_list() {
    static const std::string s = [] {
        std::string r;
        for (int k = 0; k < kOptCount; ++k) r += std::string(kOptName[k]) + ": " + kOptDoc[k] + "\n";
        return r;
    }();
    return s.c_str();
}

}  // namespace crf

extern "C" {

const char *crf_last_error(void) { return crf::g_err.c_str(); }
int crf_debug_set(const char *key, int value) { return crf::opt_set(key, value, false); }
int crf_debug_unset(const char *key) { return crf::opt_set(key, 0, true); }
const char *crf_debug_list(void) { return crf::opt_list(); }
const char *crf_version(void) { return "ctc_crf_hip 0.1.0 (gfx950)"; }

}  // extern "C"
