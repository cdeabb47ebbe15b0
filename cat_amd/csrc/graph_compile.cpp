// cat_amd/csrc/graph_compile.cpp -- the "graph compiler": turns the arc list of the denominator graph into the tables the gfx950 kernels
// stream.  compile_graph is the list of its steps: validate, re-gauge weight-pushed graphs, number the pairs (crf_internal.h: PairGraph),
// build the generic tables (sliced ELL in both directions, pair and row descriptors, grad-pass chunks) and the utterance-minor tables
// (arc_streams.cpp), fill the HostGraph, upload, and hand the pair graph to the register-resident layouts (res_layout.cpp).
//
// Replaces the table construction + upload of the reference's Init, den_calculate.cu:288-392 (one flat arc array per direction with a
// per-state index, copied to every GPU).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>

#include "../../include/ctc_crf_hip.h"
#include "crf_internal.h"

namespace crf {

namespace {

struct EllHost {
    std::vector<uint4> arcs;
    std::vector<int> slice_off, slice_w2, wave_off, wave_slices;
    std::vector<int> row_of;  // row position -> original row id (-1 padding)
    int64_t padded_arcs = 0;
    int64_t conflict_cycles = 0;  // gathers that land on an already-used bank (extra LDS cycles)
};

// rows[r] = list of (idx, w).  Rows are sorted by degree (descending, stable) and cut into slices
// of 64; each slice is as wide as its first (longest) row, rounded up to an even arc count.
EllHost build_ell(const ArcRows &rows) {
    EllHost e;
    const int R = (int)rows.size();
    std::vector<int> order(R);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rows[a].size() > rows[b].size(); });
    const int nsl = (R + kWave - 1) / kWave;
    e.row_of.assign((size_t)nsl * kWave, -1);
    for (int i = 0; i < R; ++i) e.row_of[i] = order[i];
    e.slice_off.resize(nsl);
    e.slice_w2.resize(nsl);
    for (int j = 0; j < nsl; ++j) {
        int wmax = (int)rows[order[(size_t)j * kWave]].size();
        int w2 = (wmax + 1) / 2;
        if (w2 > 2) w2 = (w2 + 3) & ~3;  // ell_row_sum streams groups of four elements
        e.slice_off[j] = (int)e.arcs.size();
        e.slice_w2[j] = w2;
        e.arcs.resize(e.arcs.size() + (size_t)w2 * kWave, uint4{0u, 0u, 0u, 0u});
        // Column assignment.  Column c of the slice is ONE ds_read_b32 gather per wave, serviced in
        // two 32-lane halves over 32 banks (bank = idx mod 32, MI355X_MICROARCH.md LDS table).  The
        // order of a row's arcs is free, so pick it greedily per column: lanes with the fewest arcs
        // left choose first, each takes the arc whose bank is least used in its half (equal idx =
        // broadcast, free).  Summation order changes, the sum is the same up to fp32 rounding.
        ArcRows rem(kWave);
        for (int lane = 0; lane < kWave; ++lane) {
            int r = e.row_of[(size_t)j * kWave + lane];
            if (r >= 0) rem[lane] = rows[r];
        }
        for (int c = 0; c < 2 * w2; ++c) {
            for (int half = 0; half < 2; ++half) {
                int used[32];
                int occupant[32];
                for (int b = 0; b < 32; ++b) { used[b] = 0; occupant[b] = -1; }
                int lanes[32];
                for (int l = 0; l < 32; ++l) lanes[l] = half * 32 + l;
                std::stable_sort(lanes, lanes + 32, [&](int a, int b) { return rem[a].size() < rem[b].size(); });
                for (int li = 0; li < 32; ++li) {
                    const int lane = lanes[li];
                    auto &rv = rem[lane];
                    if (rv.empty()) continue;
                    size_t best = 0;
                    int best_cost = 1 << 30;
                    for (size_t k = 0; k < rv.size(); ++k) {
                        const int bank = rv[k].first & 31;
                        const int cost = (occupant[bank] == rv[k].first) ? 0 : used[bank];
                        if (cost < best_cost) { best_cost = cost; best = k; if (cost == 0) break; }
                    }
                    const auto arc = rv[best];
                    rv.erase(rv.begin() + (long)best);
                    const int bank = arc.first & 31;
                    if (occupant[bank] != arc.first) { used[bank]++; if (occupant[bank] < 0) occupant[bank] = arc.first; }
                    e.conflict_cycles += (best_cost > 0) ? 1 : 0;
                    uint4 &a = e.arcs[(size_t)e.slice_off[j] + (size_t)(c / 2) * kWave + lane];
                    if (c & 1) { a.z = (uint32_t)arc.first; a.w = wbits(arc.second); }
                    else { a.x = (uint32_t)arc.first; a.y = wbits(arc.second); }
                }
            }
        }
        // padding arcs have weight 0; give them the index the first lane of their half reads in the same
        // column, so the padded gather is a broadcast and costs no extra bank cycle
        for (int c = 0; c < 2 * w2; ++c)
            for (int half = 0; half < 2; ++half) {
                uint32_t bidx = 0;
                bool have = false;
                for (int l = 0; l < 32 && !have; ++l) {
                    const uint4 &a = e.arcs[(size_t)e.slice_off[j] + (size_t)(c / 2) * kWave + half * 32 + l];
                    const uint32_t wb = (c & 1) ? a.w : a.y;
                    if (wb != 0u) { bidx = (c & 1) ? a.z : a.x; have = true; }
                }
                for (int l = 0; l < 32; ++l) {
                    uint4 &a = e.arcs[(size_t)e.slice_off[j] + (size_t)(c / 2) * kWave + half * 32 + l];
                    if (c & 1) { if (a.w == 0u) a.z = bidx; }
                    else { if (a.y == 0u) a.x = bidx; }
                }
            }
        e.padded_arcs += (int64_t)w2 * 2 * kWave;
    }
    // longest-processing-time assignment of slices (already sorted by width) to the waves
    std::vector<int64_t> load(kChainWaves, 0);
    std::vector<std::vector<int>> lists(kChainWaves);
    for (int j = 0; j < nsl; ++j) {
        int best = 0;
        for (int wv = 1; wv < kChainWaves; ++wv)
            if (load[wv] < load[best]) best = wv;
        lists[best].push_back(j);
        load[best] += e.slice_w2[j] + 4;  // +4: per-slice fixed cost (row epilogue)
    }
    e.wave_off.assign(kChainWaves + 1, 0);
    for (int wv = 0; wv < kChainWaves; ++wv) {
        e.wave_off[wv + 1] = e.wave_off[wv] + (int)lists[wv].size();
        for (int j : lists[wv]) e.wave_slices.push_back(j);
    }
    return e;
}

int upload_ell(HostGraph *h, const EllHost &e, EllDev *d) {
    int rc;
    if ((rc = upload(h, e.arcs, &d->arcs))) return rc;
    if ((rc = upload(h, e.slice_off, &d->slice_off))) return rc;
    if ((rc = upload(h, e.slice_w2, &d->slice_w2))) return rc;
    if ((rc = upload(h, e.wave_off, &d->wave_off))) return rc;
    if ((rc = upload(h, e.wave_slices, &d->wave_slices))) return rc;
    d->nslices = (int)e.slice_off.size();
    return CRF_OK;
}

}  // namespace

// One observation of the re-gauging: the states key >> 32 < key & 0xffffffff meet in a row with log-weight difference d.
struct GaugeObs { uint64_t key; double d; };
typedef std::map<std::pair<int, int>, std::vector<int>> ArcsOfRow;   // (label, dst) -> arcs

static void observe_all_pairs(const ArcsOfRow &rows, const int32_t *src, const std::vector<float> &w, std::vector<GaugeObs> &obs) {
    // every pair of states that meets in a row (quadratic in the row length: graphs up to a few hundred thousand arcs)
    for (auto &kv : rows) {
        const std::vector<int> &a = kv.second;
        if (a.size() < 2 || a.size() > 512) continue;
        for (size_t u = 0; u < a.size(); ++u)
            for (size_t v = u + 1; v < a.size(); ++v) {
                int s1 = src[a[u]], s2 = src[a[v]];
                double d = (double)w[(size_t)a[u]] - (double)w[(size_t)a[v]];
                if (s1 == s2 || !std::isfinite(d)) continue;
                if (s1 > s2) { std::swap(s1, s2); d = -d; }
                obs.push_back({(uint64_t)s1 << 32 | (unsigned)s2, d});
            }
    }
}

static void observe_minhashed_pairs(int64_t S, int64_t A, const ArcsOfRow &rows, const int32_t *src, const std::vector<float> &w, std::vector<GaugeObs> &obs) {
    // Large graphs (config #5: 4.3 M arcs in rows of 64 -- 134 M pairs, minutes of sorting): the two states of a history
    // feed the SAME rows but one each, so they are found as near-duplicates -- twelve min-hashes over the set of rows a state
    // feeds (two sets that differ in two of d + 2 elements share a min-hash with probability d / (d + 2)); only states that
    // collide in one of them are compared, arc list against arc list.  O(A log A).
    std::vector<int> rid((size_t)A);
    { int r = 0; for (auto &kv : rows) { for (int k : kv.second) rid[(size_t)k] = r; ++r; } }
    std::vector<int> order((size_t)A);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int x, int y) { return src[x] != src[y] ? src[x] < src[y] : rid[(size_t)x] < rid[(size_t)y]; });
    std::vector<int64_t> off((size_t)S + 1, 0);
    for (int64_t k = 0; k < A; ++k) ++off[(size_t)src[k] + 1];
    for (int64_t q = 0; q < S; ++q) off[(size_t)q + 1] += off[(size_t)q];
    constexpr int NH = 12;
    auto mix = [](uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x; };
    std::vector<uint64_t> pairs;
    std::vector<std::pair<uint64_t, int>> mh((size_t)S);
    for (int j = 0; j < NH; ++j) {
        for (int64_t q = 0; q < S; ++q) {
            uint64_t m = ~0ull;
            for (int64_t i = off[(size_t)q]; i < off[(size_t)q + 1]; ++i) m = std::min(m, mix((uint64_t)rid[(size_t)order[(size_t)i]] * 0x9e3779b97f4a7c15ull + (uint64_t)j * 0x632be59bd9b4e019ull));
            mh[(size_t)q] = {m, (int)q};
        }
        std::sort(mh.begin(), mh.end());
        for (size_t i = 0; i < mh.size();) {
            size_t e = i;
            while (e < mh.size() && mh[e].first == mh[i].first) ++e;
            if (mh[i].first != ~0ull && e - i >= 2 && e - i <= 16)
                for (size_t u = i; u < e; ++u)
                    for (size_t v = u + 1; v < e; ++v) pairs.push_back((uint64_t)std::min(mh[u].second, mh[v].second) << 32 | (unsigned)std::max(mh[u].second, mh[v].second));
            i = e;
        }
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    for (uint64_t key : pairs) {
        const int s1 = (int)(key >> 32), s2 = (int)(key & 0xffffffffu);
        int64_t i = off[(size_t)s1], j = off[(size_t)s2];
        const int64_t ie = off[(size_t)s1 + 1], je = off[(size_t)s2 + 1];
        while (i < ie && j < je) {
            const int a1 = order[(size_t)i], a2 = order[(size_t)j];
            if (rid[(size_t)a1] < rid[(size_t)a2]) ++i;
            else if (rid[(size_t)a1] > rid[(size_t)a2]) ++j;
            else {
                const double d = (double)w[(size_t)a1] - (double)w[(size_t)a2];
                if (std::isfinite(d)) obs.push_back({key, d});
                ++i; ++j;
            }
        }
    }
}

// RE-GAUGING of weight-pushed graphs.  A den_lm is CTC topology o LM: the two states (g, blank) and (g, token) of an LM
// history feed the same rows with the same weights, which is what the factored layout lives on (res_layout.cpp:
// build_factored).  A tool that PUSHES weights (w' = w + V(dst) - V(src), final' = final - V, V(start) = 0: every path
// weight unchanged) destroys the equality -- the two weights into a row then differ by the constant V(token state) -
// V(blank state).  Path weights are invariant under ANY such potential, so the compiler may choose its own: states that
// share >= 2 rows with a CONSTANT log-weight difference d get potentials that make the weights equal again (g[s2] = -d;
// w~ = w + g[dst] - g[src], start~ = start + g, end~ = end - g), and the now-equal weights are snapped to the same bits.
// Nothing happens to graphs that need nothing (all differences zero).  Returns true when the weights were changed.
static bool regauge_pushed(int64_t S, int64_t A, const int32_t *src, const int32_t *dst, const int32_t *lab,
                           std::vector<float> &w, std::vector<float> &start_w, std::vector<float> &end_w) {
    if (opt_on(kOpt_no_regauge)) return false;
    ArcsOfRow rows;
    for (int64_t k = 0; k < A; ++k) rows[{(int)lab[k], (int)dst[k]}].push_back((int)k);
    typedef GaugeObs Obs;
    std::vector<Obs> obs;
    int64_t nobs = 0;
    for (auto &kv : rows) { const int64_t n = (int64_t)kv.second.size(); if (n >= 2 && n <= 512) nobs += n * (n - 1) / 2; }
    if (nobs <= 30000000 && !opt_on(kOpt_regauge_minhash)) observe_all_pairs(rows, src, w, obs);
    else observe_minhashed_pairs(S, A, rows, src, w, obs);
    std::sort(obs.begin(), obs.end(), [](const Obs &x, const Obs &y) { return x.key < y.key || (x.key == y.key && x.d < y.d); });
    struct Cand { uint64_t key; int n; double d; };
    std::vector<Cand> cand;
    for (size_t i = 0; i < obs.size();) {
        size_t j = i;
        while (j < obs.size() && obs[j].key == obs[i].key) ++j;
        // the difference MOST of the common rows agree on (a pair may also meet in a row where its weights have nothing to
        // do with each other: the self-loop of (g, token) beside the arc from (g, blank) when the history maps to itself)
        size_t best_a = i, best_n = 0;
        for (size_t a = i, b = i; a < j; ++a) {
            while (b < j && obs[b].d - obs[a].d <= 1e-4) ++b;
            if (b - a > best_n) { best_n = b - a; best_a = a; }
        }
        if (best_n >= 2) {
            double sum = 0.0;
            for (size_t a = best_a; a < best_a + best_n; ++a) sum += obs[a].d;
            cand.push_back({obs[i].key, (int)best_n, sum / (double)best_n});
        }
        i = j;
    }
    std::stable_sort(cand.begin(), cand.end(), [](const Cand &x, const Cand &y) { return x.n > y.n; });
    std::vector<int> mate((size_t)S, -1);
    std::vector<double> g((size_t)S, 0.0);
    int64_t moved = 0, matched = 0;
    for (const Cand &c : cand) {
        const int s1 = (int)(c.key >> 32), s2 = (int)(c.key & 0xffffffffu);
        if (mate[s1] >= 0 || mate[s2] >= 0) continue;
        mate[s1] = s2; mate[s2] = s1;
        g[s2] = -c.d;                                     // w(s1 -> d) - g[s1] == w(s2 -> d) - g[s2], g[s1] = 0
        ++matched;
        if (std::fabs(c.d) > 1e-6) ++moved;
    }
    if (opt_on(kOpt_verbose))
        fprintf(stderr, "[regauge] %lld candidate pairs, %lld matched, %lld with a non-zero difference (S = %lld)\n", (long long)cand.size(), (long long)matched, (long long)moved, (long long)S);
    if (moved * 8 < S) return false;                       // not a pushed T o LM graph (or nothing to undo)
    for (int64_t k = 0; k < A; ++k) w[(size_t)k] = (float)((double)w[(size_t)k] + g[dst[k]] - g[src[k]]);
    for (int64_t s = 0; s < S; ++s) {
        if (std::isfinite(start_w[(size_t)s])) start_w[(size_t)s] = (float)((double)start_w[(size_t)s] + g[s]);
        if (std::isfinite(end_w[(size_t)s])) end_w[(size_t)s] = (float)((double)end_w[(size_t)s] - g[s]);
    }
    // Snap the weights of mates in a common row to the same bits -- within the ROUNDING of the pushed weights only (the file
    // holds fp32 sums w + V(dst) - V(src): a few ulp of the weight's magnitude); a pair that differs by more is left alone
    // (it then simply does not factor), so no path weight moves by more than float rounding.
    double max_snap = 0.0;
    for (auto &kv : rows) {
        const std::vector<int> &a = kv.second;
        if (a.size() < 2 || a.size() > 512) continue;   // (quadratic in the row length)
        for (size_t u = 0; u < a.size(); ++u)
            for (size_t v = u + 1; v < a.size(); ++v) {
                if (mate[src[a[u]]] != src[a[v]]) continue;
                const double wu = w[(size_t)a[u]], wv = w[(size_t)a[v]], df = std::fabs(wu - wv);
                if (df <= 4e-6 * std::max(1.0, std::max(std::fabs(wu), std::fabs(wv)))) { w[(size_t)a[v]] = w[(size_t)a[u]]; max_snap = std::max(max_snap, df); }
            }
    }
    if (opt_on(kOpt_verbose)) fprintf(stderr, "[regauge] largest snapped log-weight difference %.3g\n", max_snap);
    return true;
}

// Grad-pass lists are label-sorted and cut into chunks of at most `cap` entries within one label (labels[i]: the label of entry i):
// chunk_off [NC + 1] = the chunks' ends, lab_chunk_off [max_label + 2] = the chunk range of each label.  Returns NC; with both
// outputs null it only counts.
int cut_label_chunks(const std::vector<int> &labels, int max_label, int cap, std::vector<int> *chunk_off, std::vector<int> *lab_chunk_off) {
    const int n = (int)labels.size();
    int nc = 0, r = 0;
    if (chunk_off) { chunk_off->assign(1, 0); lab_chunk_off->assign((size_t)max_label + 2, 0); }
    for (int v = 0; v <= max_label; ++v) {
        if (chunk_off) (*lab_chunk_off)[(size_t)v] = nc;
        int e = r;
        while (e < n && labels[(size_t)e] == v) ++e;
        for (int c = r; c < e; c += cap, ++nc) if (chunk_off) chunk_off->push_back(std::min(e, c + cap));
        r = e;
    }
    if (chunk_off) (*lab_chunk_off)[(size_t)max_label + 1] = nc;
    return nc;
}

namespace {

// Step 1: sizes, endpoints and labels of the arc list; *max_label = the largest label.
int validate_arcs(int64_t S, int64_t A, const int32_t *src, const int32_t *dst, const int32_t *lab, int *max_label) {
    if (S <= 0 || S > INT32_MAX / 4 || A < 0 || A > INT32_MAX / 4) { set_error("graph size out of range"); return CRF_ERR_UNSUPPORTED; }
    *max_label = 0;
    for (int64_t k = 0; k < A; ++k) {
        if (src[k] < 0 || src[k] >= S || dst[k] < 0 || dst[k] >= S) { set_error("arc endpoint out of range"); return CRF_ERR_ARG; }
        if (lab[k] < 0) { set_error("negative label (epsilon ilabel) on an arc"); return CRF_ERR_FORMAT; }
        *max_label = std::max(*max_label, (int)lab[k]);
    }
    return CRF_OK;
}

// Step 3: pairs = distinct (label, destination), numbered in that order (std::map: deterministic); weights exponentiated once.
PairGraph number_pairs(int64_t S, int64_t A, const int32_t *src, const int32_t *dst, const int32_t *lab, int max_label,
                       const std::vector<float> &w, const std::vector<float> &start_w, const std::vector<float> &end_w) {
    PairGraph g;
    std::map<std::pair<int, int>, int> pair_id;
    for (int64_t k = 0; k < A; ++k) pair_id.emplace(std::make_pair((int)lab[k], (int)dst[k]), 0);
    g.S = (int)S; g.P = (int)pair_id.size(); g.max_label = max_label;
    g.pair_dst.resize(g.P); g.pair_lab.resize(g.P);
    int n = 0;
    for (auto &kv : pair_id) { kv.second = n; g.pair_lab[n] = kv.first.first; g.pair_dst[n] = kv.first.second; ++n; }
    g.in_arcs_of_pair.resize(g.P); g.out_arcs_of_state.resize((size_t)S);
    g.arc_pair.resize((size_t)A); g.w_lin.resize((size_t)A);
    for (int64_t k = 0; k < A; ++k) {
        const int p = pair_id[{(int)lab[k], (int)dst[k]}];
        const float e = expf(w[(size_t)k]);
        g.arc_pair[(size_t)k] = p; g.w_lin[(size_t)k] = e;
        g.in_arcs_of_pair[p].push_back({(int)src[k], e});
        g.out_arcs_of_state[src[k]].push_back({p, e});
    }
    g.start_lin.resize((size_t)S); g.end_lin.resize((size_t)S);
    for (int64_t s = 0; s < S; ++s) { g.start_lin[s] = expf(start_w[s]); g.end_lin[s] = expf(end_w[s]); }
    return g;
}

// Step 4: the tables of the streaming ("generic") kernels.  From here on a pair's id is its row in the forward ELL (GraphDev).
struct GenericTables {
    EllHost fwd, bwd;                    // rows = pairs, arc index = source state / rows = states, arc index = pair
    std::vector<int2> pair_meta;         // [Pr]
    std::vector<int4> bwd_row_meta;      // [Sr]
    std::vector<int> st_pair_off, st_pairs, perm, chunk_off, lab_chunk_off;
};
GenericTables build_generic_tables(const PairGraph &g) {
    GenericTables t;
    const int S = g.S, P = g.P;
    t.fwd = build_ell(g.in_arcs_of_pair);
    const int Pr = (int)t.fwd.row_of.size();
    std::vector<int> row_of_pair(P), pair_dst(Pr, -1), pair_lab(Pr, 0);
    for (int r = 0; r < Pr; ++r) {
        const int p = t.fwd.row_of[r];
        if (p >= 0) { row_of_pair[p] = r; pair_dst[r] = g.pair_dst[p]; pair_lab[r] = g.pair_lab[p]; }
    }
    ArcRows brows = g.out_arcs_of_state;
    for (auto &row : brows) for (auto &a : row) a.first = row_of_pair[a.first];
    t.bwd = build_ell(brows);
    const int Sr = (int)t.bwd.row_of.size();
    // pairs of each destination state
    t.st_pair_off.assign((size_t)S + 1, 0); t.st_pairs.resize(P);
    for (int r = 0; r < Pr; ++r) if (pair_dst[r] >= 0) t.st_pair_off[(size_t)pair_dst[r] + 1]++;
    for (int s = 0; s < S; ++s) t.st_pair_off[(size_t)s + 1] += t.st_pair_off[s];
    std::vector<int> fill(t.st_pair_off.begin(), t.st_pair_off.end() - 1);
    for (int r = 0; r < Pr; ++r) if (pair_dst[r] >= 0) t.st_pairs[fill[pair_dst[r]]++] = r;
    // grad pass: pair ids sorted by (label, pair id); chunks of <= kChunk within a label
    t.perm.reserve(P);
    for (int r = 0; r < Pr; ++r) if (pair_dst[r] >= 0) t.perm.push_back(r);
    std::stable_sort(t.perm.begin(), t.perm.end(), [&](int a, int b) { return pair_lab[a] < pair_lab[b]; });
    std::vector<int> perm_lab;
    for (int r : t.perm) perm_lab.push_back(pair_lab[r]);
    cut_label_chunks(perm_lab, g.max_label, kChunk, &t.chunk_off, &t.lab_chunk_off);
    // label | (1 << 16) when the pair is the only one into its destination state (plain LDS store)
    t.pair_meta.resize(Pr);
    for (int r = 0; r < Pr; ++r) {
        const bool sole = pair_dst[r] >= 0 && t.st_pair_off[(size_t)pair_dst[r] + 1] - t.st_pair_off[pair_dst[r]] == 1;
        t.pair_meta[r] = int2{pair_dst[r], pair_lab[r] | (sole ? 1 << 16 : 0)};
    }
    t.bwd_row_meta.resize(Sr);
    for (int r = 0; r < Sr; ++r) {
        const int st = t.bwd.row_of[r];
        int4 m{-1, 0, 0, 0};
        if (st >= 0) {
            m.x = st;
            m.y = t.st_pair_off[(size_t)st + 1] - t.st_pair_off[st];
            if (m.y > 0) { m.z = t.st_pairs[t.st_pair_off[st]]; m.w = pair_lab[m.z]; }
        }
        t.bwd_row_meta[r] = m;
    }
    return t;
}

// Step 6: the HostGraph's scalars, statistics and kept host copies.
void fill_host_graph(HostGraph *h, int device, const PairGraph &g, const GenericTables &t, const BatchHost &bt, FacBatchH &&fb,
                     int64_t A, const int32_t *src, const int32_t *dst, const int32_t *lab, bool regauged) {
    h->device = device < 0 ? -1 : device;   // (-1: host-only compile for diagnostics / CPU tests -- tables are built, nothing is uploaded)
    h->S = g.S; h->A = A; h->P = g.P; h->regauged = regauged ? 1 : 0;
    if (device >= 0) { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) h->ncu = n; else (void)hipGetLastError(); }
    h->fwd_padded_arcs = t.fwd.padded_arcs; h->bwd_padded_arcs = t.bwd.padded_arcs;
    h->fwd_conflicts = t.fwd.conflict_cycles; h->bwd_conflicts = t.bwd.conflict_cycles;
    for (auto &r : g.in_arcs_of_pair) h->max_in_deg = std::max(h->max_in_deg, (int)r.size());
    for (auto &r : g.out_arcs_of_state) h->max_out_deg = std::max(h->max_out_deg, (int)r.size());
    GraphDev &d = h->dev;
    d.S = g.S; d.A = (int)A; d.P = g.P; d.Pr = (int)t.fwd.row_of.size(); d.Sr = (int)t.bwd.row_of.size(); d.max_label = g.max_label;
    d.NC = (int)t.chunk_off.size() - 1;
    h->hb_farcs = bt.farcs; h->hb_barcs = bt.barcs; h->hb_frow = bt.frow; h->hb_brow = bt.brow;   // (kept: arc streams are cut from them on first use)
    h->hb_frow_d = bt.frow_d; h->hb_brow_s = bt.brow_s;
    h->fb = std::move(fb);
    if (A <= (1 << 20)) {   // (kept for the CPU emulations of the layouts: their reference is the recursion over these arcs)
        h->h_src.assign(src, src + A); h->h_dst.assign(dst, dst + A); h->h_lab.assign(lab, lab + A);
        h->h_w = g.w_lin; h->h_start = g.start_lin; h->h_end = g.end_lin;
    }
}

// The one upload: every table of steps 4 and 5.  A host-only graph keeps null pointers (and bat.ok = 0: no utterance-minor kernels).
int upload_tables(HostGraph *h, const PairGraph &g, const GenericTables &t, const BatchHost &bt) {
    if (h->device < 0) return CRF_OK;
    GraphDev &d = h->dev;
    int rc;
    if ((rc = upload_ell(h, t.fwd, &d.fwd)) || (rc = upload_ell(h, t.bwd, &d.bwd)) ||
        (rc = upload(h, t.pair_meta, &d.pair_meta)) || (rc = upload(h, t.bwd_row_meta, &d.bwd_row_meta)) ||
        (rc = upload(h, t.st_pair_off, &d.st_pair_off)) || (rc = upload(h, t.st_pairs, &d.st_pairs)) ||
        (rc = upload(h, g.start_lin, &d.start_lin)) || (rc = upload(h, g.end_lin, &d.end_lin)) ||
        (rc = upload(h, t.perm, &d.perm)) || (rc = upload(h, t.chunk_off, &d.chunk_off)) || (rc = upload(h, t.lab_chunk_off, &d.lab_chunk_off)) ||
        (rc = upload(h, bt.farcs, &d.bat.farcs)) || (rc = upload(h, bt.frow_d, &d.bat.frow_d)) || (rc = upload(h, bt.frow, &d.bat.frow)) ||
        (rc = upload(h, bt.stp, &d.bat.stp)) || (rc = upload(h, bt.barcs, &d.bat.barcs)) || (rc = upload(h, bt.brow_s, &d.bat.brow_s)) ||
        (rc = upload(h, bt.brow, &d.bat.brow)) || (rc = upload(h, bt.lab_off, &d.bat.lab_off))) return rc;
    d.bat.ok = 1;
    return CRF_OK;
}

}  // namespace

int compile_graph(int64_t S, int64_t A, const int32_t *src, const int32_t *dst, const int32_t *lab,
                  const float *w_in, const float *start_in, const float *end_in, int device, HostGraph **out) {
    int max_label = 0, rc;
    if ((rc = validate_arcs(S, A, src, dst, lab, &max_label))) return rc;
    // the compiler's own potentials for weight-pushed graphs (regauge_pushed): every table below is built from these weights
    std::vector<float> w(w_in, w_in + A), start_w(start_in, start_in + S), end_w(end_in, end_in + S);
    const bool regauged = regauge_pushed(S, A, src, dst, lab, w, start_w, end_w);
    const PairGraph g = number_pairs(S, A, src, dst, lab, max_label, w, start_w, end_w);
    const GenericTables t = build_generic_tables(g);
    BatchHost bt;
    FacBatchH fb;
    build_batch_tables(g, &bt, &fb);
    auto *h = new HostGraph();
    fill_host_graph(h, device, g, t, bt, std::move(fb), A, src, dst, lab, regauged);
    int prev = 0;
    if (device >= 0 && (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess)) {
        set_error(std::string("cannot select device ") + std::to_string(device));
        delete h;
        return CRF_ERR_HIP;
    }
    rc = upload_tables(h, g, t, bt);
    if (!rc) rc = build_resident(h, g);
    if (!rc) rc = build_factored(h, g);
    if (device >= 0) (void)hipSetDevice(prev);
    if (rc) {
        for (void *p : h->allocs) (void)hipFree(p);
        delete h;
        return rc;
    }
    *out = h;
    return CRF_OK;
}

}  // namespace crf

extern "C" {

int crf_graph_create_from_arcs(int64_t S, int64_t A, const int32_t *src, const int32_t *dst,
                               const int32_t *lab, const float *w, const float *start_w,
                               const float *end_w, int device, crf_graph **out) {
    if (!out || !start_w || !end_w || (A > 0 && (!src || !dst || !lab || !w))) { crf::set_error("null argument"); return CRF_ERR_ARG; }
    crf::HostGraph *h = nullptr;
    int rc = crf::compile_graph(S, A, src, dst, lab, w, start_w, end_w, device, &h);
    if (rc) return rc;
    *out = new crf_graph{h};
    return CRF_OK;
}

void crf_graph_destroy(crf_graph *g) {
    if (!g) return;
    if (g->h) {
        // a host-only graph (device < 0) owns no device memory and makes no HIP call: hipSetDevice(-1) fails, and the runtime keeps
        // hipErrorInvalidDevice as the thread's last error, which the next launch check -- the library's or torch's -- then reports
        if (g->h->device >= 0) {
            int prev = 0;
            bool sw = hipGetDevice(&prev) == hipSuccess && hipSetDevice(g->h->device) == hipSuccess;
            for (void *p : g->h->allocs) (void)hipFree(p);
            if (sw) (void)hipSetDevice(prev);
        }
        for (crf::StreamDev *sd : g->h->streams) delete sd;
        delete g->h;
    }
    delete g;
}

int crf_graph_dims(const crf_graph *g, int64_t *S, int64_t *A, int64_t *P, int64_t *max_label) {
    if (!g || !g->h) { crf::set_error("null graph"); return CRF_ERR_ARG; }
    if (S) *S = g->h->S;
    if (A) *A = g->h->A;
    if (P) *P = g->h->P;
    if (max_label) *max_label = g->h->dev.max_label;
    return CRF_OK;
}

int crf_graph_stats(const crf_graph *g, int64_t *out, int n) {
    if (!g || !g->h || !out) { crf::set_error("null argument"); return CRF_ERR_ARG; }
    const crf::HostGraph *h = g->h;
    int64_t fac_geom, fac_chunks;
    crf::fac_geom_public(h, &fac_geom, &fac_chunks);
    const int64_t v[27] = {h->S, h->A, h->P, h->dev.Pr, h->dev.Sr, h->fwd_padded_arcs, h->bwd_padded_arcs,
                           h->fwd_conflicts, h->bwd_conflicts, (int64_t)h->max_in_deg * 100000 + h->max_out_deg,
                           h->res_stats.K, h->res_stats.slots_f, h->res_stats.slots_b, h->res_stats.conflicts_f,
                           h->res_stats.conflicts_b, (int64_t)h->dev.res.f.R * 100000 + h->dev.res.b.R,
                           h->fac_stats.ok, h->fac_stats.matched, (int64_t)h->regauged, h->fac_stats.tail,
                           h->fac_stats.slots_f, h->fac_stats.slots_b, h->fac_stats.fused,
                           h->fac_stats.Gf * 100000 + h->fac_stats.Gb,
                           fac_geom, fac_chunks,
                           h->facp.ok};
    for (int i = 0; i < n && i < 27; ++i) out[i] = v[i];
    return CRF_OK;
}

int crf_debug_fac_emulate(const crf_graph *g, int T, unsigned seed, double *out3) {
    if (!g || !g->h || !out3 || T < 1) { crf::set_error("bad argument"); return CRF_ERR_ARG; }
    return crf::debug_emulate_factored(g->h, T, seed, out3, crf::opt_on(crf::kOpt_emu_facp) ? 1 : 0);
}

int crf_debug_res_emulate(const crf_graph *g, int T, unsigned seed, double *out3) {
    if (!g || !g->h || !out3 || T < 1) { crf::set_error("bad argument"); return CRF_ERR_ARG; }
    return crf::debug_emulate_resident(g->h, T, seed, out3);
}

}  // extern "C"
