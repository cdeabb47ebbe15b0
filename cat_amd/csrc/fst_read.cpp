// cat_amd/csrc/fst_read.cpp -- OpenFst-binary reader of the denominator graph (no OpenFst) and crf_graph_create.
//
// Replaces reference src/ctc_crf/gpu_den/fst_read.cc:11-62 (ReadFst on top of OpenFst 1.6.7, which is not vendored).
// Conventions are the reference's (fst_read.cc:40-60): label = ilabel-1, weight = -cost,
// end_weight = -Final, start_weight[start] = 0.  Epsilon input labels are rejected (the reference
// would read logits[-1], fst_read.cc:55-56).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/ctc_crf_hip.h"
#include "crf_internal.h"

namespace crf {

namespace {
struct Cursor {
    const unsigned char *p;
    size_t n, off = 0;
    bool ok = true;
    template <typename T>
    T get() {
        T v{};
        if (off + sizeof(T) > n) { ok = false; return v; }
        memcpy(&v, p + off, sizeof(T));
        off += sizeof(T);
        return v;
    }
    std::string str() {
        int32_t len = get<int32_t>();
        if (!ok || len < 0 || off + (size_t)len > n) { ok = false; return {}; }
        std::string s((const char *)p + off, (size_t)len);
        off += (size_t)len;
        return s;
    }
    void skip_symtab() {  // OpenFst SymbolTable binary: magic, name, available_key, size, entries
        get<int32_t>(); str(); get<int64_t>();
        int64_t cnt = get<int64_t>();
        for (int64_t i = 0; ok && i < cnt; ++i) { str(); get<int64_t>(); }
    }
};

int read_fst_file(const char *path, int64_t *S, std::vector<int32_t> *src, std::vector<int32_t> *dst,
                  std::vector<int32_t> *lab, std::vector<float> *w, std::vector<float> *start_w,
                  std::vector<float> *end_w) {
    FILE *f = fopen(path, "rb");
    if (!f) { set_error(std::string("cannot open den_lm: ") + path); return CRF_ERR_IO; }
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> buf((size_t)std::max(0L, sz));
    size_t got = buf.empty() ? 0 : fread(buf.data(), 1, buf.size(), f);
    fclose(f);
    if (got != buf.size()) { set_error(std::string("short read: ") + path); return CRF_ERR_IO; }
    Cursor c{buf.data(), buf.size()};
    if (c.get<uint32_t>() != 0x7eb2fdd6u) { set_error(std::string(path) + ": not an OpenFst binary (bad magic)"); return CRF_ERR_FORMAT; }
    std::string fsttype = c.str(), arctype = c.str();
    if (fsttype != "vector" || arctype != "standard") {
        set_error(std::string(path) + ": need fst type vector/standard, got " + fsttype + "/" + arctype);
        return CRF_ERR_FORMAT;
    }
    c.get<int32_t>();  // version
    int32_t flags = c.get<int32_t>();
    c.get<uint64_t>();  // properties
    int64_t start = c.get<int64_t>();
    int64_t ns = c.get<int64_t>();
    c.get<int64_t>();  // narcs (0 in VectorFst headers; arcs are counted per state)
    if (flags & 1) c.skip_symtab();
    if (flags & 2) c.skip_symtab();
    if (!c.ok || ns <= 0 || ns > INT32_MAX || start < 0 || start >= ns) {
        set_error(std::string(path) + ": corrupt header / no start state");
        return CRF_ERR_FORMAT;
    }
    *S = ns;
    start_w->assign((size_t)ns, -INFINITY);
    end_w->assign((size_t)ns, -INFINITY);
    (*start_w)[(size_t)start] = 0.f;
    for (int64_t s = 0; s < ns; ++s) {
        float fin = c.get<float>();
        int64_t na = c.get<int64_t>();
        if (!c.ok || na < 0) { set_error(std::string(path) + ": truncated state record"); return CRF_ERR_FORMAT; }
        if (fin != INFINITY) (*end_w)[(size_t)s] = -fin;
        for (int64_t k = 0; k < na; ++k) {
            int32_t il = c.get<int32_t>();
            c.get<int32_t>();
            float cost = c.get<float>();
            int32_t nx = c.get<int32_t>();
            if (!c.ok) { set_error(std::string(path) + ": truncated arc record"); return CRF_ERR_FORMAT; }
            if (il <= 0) { set_error(std::string(path) + ": epsilon / negative input label on an arc (den_lm must be epsilon-free)"); return CRF_ERR_FORMAT; }
            if (nx < 0 || nx >= ns) { set_error(std::string(path) + ": arc to a non-existent state"); return CRF_ERR_FORMAT; }
            src->push_back((int32_t)s); dst->push_back(nx); lab->push_back(il - 1); w->push_back(-cost);
        }
    }
    if (src->size() > (size_t)INT32_MAX) { set_error("too many arcs"); return CRF_ERR_UNSUPPORTED; }
    return CRF_OK;
}

}  // namespace
}  // namespace crf

extern "C" {

int crf_graph_create(const char *fst_path, int device, crf_graph **out) {
    if (!fst_path || !out) { crf::set_error("null argument"); return CRF_ERR_ARG; }
    int64_t S = 0;
    std::vector<int32_t> src, dst, lab;
    std::vector<float> w, sw, ew;
    int rc = crf::read_fst_file(fst_path, &S, &src, &dst, &lab, &w, &sw, &ew);
    if (rc) return rc;
    return crf_graph_create_from_arcs(S, (int64_t)src.size(), src.data(), dst.data(), lab.data(), w.data(),
                                      sw.data(), ew.data(), device, out);
}

}  // extern "C"
