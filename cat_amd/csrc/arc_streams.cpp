// cat_amd/csrc/arc_streams.cpp -- the tables of the UTTERANCE-MINOR kernels (crf_internal.h: BatchDev, StreamDev; k_batch.hip): the CSR tables with one
// descriptor per row, the factored rows of T o LM graphs, the arc streams cut from either on first use, and the host-side checks of all three.
//
// No reference counterpart: the reference walks one flat arc array per direction, one thread per arc and utterance, with atomic adds into the
// state vector (den_calculate.cu:75-103, 189-227); these tables read every arc once per frame for a whole group of utterances.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>

#include "../../include/ctc_crf_hip.h"
#include "crf_internal.h"

namespace crf {

namespace {

// One direction's arc stream (crf_internal.h: StreamDirDev).  rows / row_st / arcs: the BatchDev tables of that direction.
struct StreamHost { std::vector<int4> tasks, meta; std::vector<int2> recs; std::vector<int> rest; };
// a stream row: NM descriptor words and its records
struct SRow { int4 m[3]; const int2 *recs; int n; };
// rows (most records first) -> bundles of AL rows -> tasks of at most `maxb` bundles and about task_steps steps
static int build_stream_rows(int AL, int UL, int task_steps, int maxb, int NM, const std::vector<SRow> &srows, StreamHost *sh) {
    constexpr int kB = kStreamBatch;
    std::vector<int4> tasks, meta;
    std::vector<int2> recs;
    const int nbund = ((int)srows.size() + AL - 1) / AL;
    // what a bundle costs a task besides its gather batches: its row epilogues (stores, ring refill), in batches of 4 steps -- the last tasks of a combo hold the
    // shortest rows, i.e. the most bundles per gather step, and were the last to reach the frame's end (profiles/round6_ab_persistent_batch.txt: 15 us where
    // the first tasks take 10): kBatEpiDefault
    const int epi = kBatEpiDefault * kB;
    int task_b0 = 0, task_batch0 = 0, task_steps_now = 0;
    auto close_task = [&](int b1) {
        if (b1 == task_b0) return;
        const int nbat = (int)(recs.size() / ((size_t)AL * kB)) - task_batch0;
        tasks.push_back(int4{task_batch0, nbat, task_b0, b1 - task_b0});
        task_b0 = b1; task_batch0 += nbat; task_steps_now = 0;
    };
    for (int b = 0; b < nbund; ++b) {
        int len = 0;
        for (int aj = 0; aj < AL; ++aj) {
            const int i = b * AL + aj;
            if (i < (int)srows.size()) len = std::max(len, srows[(size_t)i].n);
        }
        const int nbat = (len + kB - 1) / kB;             // every row of the bundle padded to whole batches
        if (task_steps_now > 0 && (task_steps_now + nbat * kB + epi > task_steps || b - task_b0 >= maxb)) close_task(b);
        for (int aj = 0; aj < AL; ++aj) {
            const int i = b * AL + aj;
            for (int q = 0; q < NM; ++q) meta.push_back(i < (int)srows.size() ? srows[(size_t)i].m[q] : int4{-1, 0, 0, 0});   // (padding row: state -1)
        }
        for (int bt = 0; bt < nbat; ++bt)
            for (int aj = 0; aj < AL; ++aj)
                for (int k = 0; k < kB; ++k) {
                    const int st = bt * kB + k, i = b * AL + aj;
                    int2 rcd{0, 0};
                    if (i < (int)srows.size() && st < srows[(size_t)i].n) {
                        rcd = srows[(size_t)i].recs[st];
                        // the kernels want entry * UL (UL utterances per entry), below 2^29 so that the byte offset fits 31 bits
                        if (rcd.x < 0 || (int64_t)rcd.x * UL >= (1ll << 29)) { set_error("arc stream: index does not fit"); return CRF_ERR_ARG; }
                        rcd.x *= UL;
                    }
                    if (k == 0 && bt == nbat - 1) rcd.x |= (int)0x80000000u;   // the bundle ends with this batch
                    recs.push_back(rcd);
                }
        task_steps_now += nbat * kB + epi;
    }
    close_task(nbund);
    recs.resize(recs.size() + 2 * kStreamRecB / sizeof(int2), int2{0, 0});   // the kernels stage whole chunks of kStreamRecB bytes, one chunk ahead
    sh->tasks = std::move(tasks); sh->meta = std::move(meta); sh->recs = std::move(recs);
    return CRF_OK;
}
static int build_stream_host(int AL, int UL, int task_steps, const std::vector<int4> &rows, const std::vector<int> &row_st,
                             const std::vector<int2> &arcs, StreamHost *sh) {
    std::vector<SRow> srows;
    std::vector<int> rest;
    for (int r = 0; r < (int)rows.size(); ++r) {
        const int4 &d = rows[(size_t)r];
        if ((d.w & 0x40000000) && d.y > d.x)               // (rows are most-arcs-first already)
            srows.push_back(SRow{{int4{row_st[(size_t)r], d.z, d.w & 0xffff, 0}, int4{-1, 0, 0, 0}, int4{0, 0, 0, 0}}, arcs.data() + d.x, d.y - d.x});
        else rest.push_back(r);
    }
    const int rc = build_stream_rows(AL, UL, task_steps, kStreamBundles, 1, srows, sh);
    sh->rest = std::move(rest);
    return rc;
}
// ... and of the factored rows (three descriptor words per row)
static std::vector<SRow> fac_stream_rows(const std::vector<FacRowH> &rows) {
    std::vector<SRow> srows;
    for (const FacRowH &r : rows)
        srows.push_back(SRow{{int4{r.st0, r.pr0, r.lab0, 0}, int4{r.st1, r.pr1, r.lab1, 0}, int4{r.x0, r.w0, r.x1, r.w1}}, r.recs.data(), (int)r.recs.size()});
    return srows;
}
static int build_stream_host_fac(int AL, int UL, int task_steps, const std::vector<FacRowH> &rows, const std::vector<int> &rest, StreamHost *sh) {
    const int rc = build_stream_rows(AL, UL, task_steps, stream_max_bundles(UL, true), 3, fac_stream_rows(rows), sh);
    sh->rest = rest;
    return rc;
}

static int upload_stream(HostGraph *h, const StreamHost &sh, StreamDirDev *out) {
    out->ntasks = (int)sh.tasks.size(); out->nrest = (int)sh.rest.size();
    int rc;
    if ((rc = upload(h, sh.tasks, &out->tasks)) || (rc = upload(h, sh.recs, &out->recs)) || (rc = upload(h, sh.meta, &out->meta)) || (rc = upload(h, sh.rest, &out->rest))) return rc;
    return CRF_OK;
}

// Host-side check of the arc streams (tests; no GPU): every row with one entering pair and at least one arc is in exactly one
// bundle of exactly one task, its records are its arcs (index * UL, weight bits) in order followed by null records, the
// end-of-bundle flag sits in the first record of the bundle's last batch for every lane group and nowhere else, a task has
// at most kStreamBundles bundles, every other row is in `rest`.  out: {tasks, rest rows, steps, arc records that are not padding}.
static int check_stream_host(int AL, int UL, const StreamHost &sh, const std::vector<int4> &rows, const std::vector<int> &row_st,
                             const std::vector<int2> &arcs, int64_t *out) {
    constexpr int kB = kStreamBatch;
    auto fail = [&](const char *why) { set_error(std::string("arc stream check: ") + why); return CRF_ERR_ARG; };
    std::vector<int> row_of_state_pair;                   // rows are identified by (state, pair id)
    std::vector<char> seen(rows.size(), 0);
    std::map<std::pair<int, int>, int> row_at;
    for (int r = 0; r < (int)rows.size(); ++r) if ((rows[(size_t)r].w & 0x40000000) && rows[(size_t)r].y > rows[(size_t)r].x) row_at[{row_st[(size_t)r], rows[(size_t)r].z}] = r;
    int64_t steps = 0, real = 0;
    int next_bundle = 0;
    for (const int4 &t : sh.tasks) {
        if (t.w < 1 || t.w > kStreamBundles) return fail("a task has no or more than 8 bundles");
        if (t.z != next_bundle) return fail("the tasks do not cover the bundles in order");
        next_bundle += t.w;
        int batch = t.x;
        for (int b = 0; b < t.w; ++b) {
            // length of this bundle: up to the batch that carries the flag
            int nbat = 0;
            for (;;) {
                if (batch + nbat >= t.x + t.y) return fail("a bundle runs past its task");
                const int2 first = sh.recs[((size_t)(batch + nbat) * AL + 0) * kB];
                ++nbat;
                if (first.x < 0) break;
            }
            for (int aj = 0; aj < AL; ++aj) {
                const int4 m = sh.meta[(size_t)(t.z + b) * AL + aj];
                int n = 0, a0 = 0;
                if (m.x >= 0) {
                    auto it = row_at.find({m.x, m.y});
                    if (it == row_at.end()) return fail("a descriptor names a row that is not a stream row");
                    const int r = it->second;
                    if (seen[(size_t)r]) return fail("a row appears twice");
                    seen[(size_t)r] = 1;
                    if ((rows[(size_t)r].w & 0xffff) != m.z) return fail("label of a descriptor");
                    n = rows[(size_t)r].y - rows[(size_t)r].x; a0 = rows[(size_t)r].x;
                    if (n > nbat * kB) return fail("a row is longer than its bundle");
                }
                for (int st = 0; st < nbat * kB; ++st) {
                    const int2 rc = sh.recs[((size_t)(batch + st / kB) * AL + aj) * kB + st % kB];
                    const bool flag = rc.x < 0, want_flag = st == (nbat - 1) * kB;
                    if (flag != want_flag) return fail("end-of-bundle flag");
                    const int idx = rc.x & 0x7fffffff;
                    if (st < n) {
                        if (idx != arcs[(size_t)a0 + st].x * UL || rc.y != arcs[(size_t)a0 + st].y) return fail("a record is not its arc");
                        ++real;
                    } else if (idx != 0 || rc.y != 0) return fail("padding record is not null");
                }
            }
            batch += nbat; steps += (int64_t)nbat * kB;
        }
        if (batch != t.x + t.y) return fail("batches of a task");
    }
    int64_t nrest = 0;
    std::vector<char> in_rest(rows.size(), 0);
    for (int r : sh.rest) { if (r < 0 || r >= (int)rows.size() || in_rest[(size_t)r]) return fail("rest list"); in_rest[(size_t)r] = 1; ++nrest; }
    for (int r = 0; r < (int)rows.size(); ++r) {
        const bool simple = (rows[(size_t)r].w & 0x40000000) && rows[(size_t)r].y > rows[(size_t)r].x;
        if (simple != (seen[(size_t)r] != 0) || simple == (in_rest[(size_t)r] != 0)) return fail("a row is in neither or both of stream and rest");
    }
    out[0] += (int64_t)sh.tasks.size(); out[1] += nrest; out[2] += steps; out[3] += real;
    return CRF_OK;
}

}  // namespace

// The utterance-minor ("batch") tables: CSR with one descriptor per row, rows in processing order (most arcs first, so the long rows of a
// launch start first); pair ids are the intermediate graph's, which are in (label, destination) order.
static void build_batch_plain(const PairGraph &g, BatchHost *bt) {
    const int S = g.S, P = g.P;
    const size_t A = g.arc_pair.size();
    bt->farcs.resize(A); bt->barcs.resize(A);
    bt->stp.resize((size_t)P); bt->frow.resize((size_t)S); bt->brow.resize((size_t)S);
    bt->frow_d.resize((size_t)S); bt->brow_s.resize((size_t)S); bt->lab_off.assign((size_t)g.max_label + 2, 0);
    std::vector<int4> &stp = bt->stp;
    std::vector<int> st_poff((size_t)S + 1, 0), bst_off((size_t)S + 1, 0);
    for (int p = 0; p < P; ++p) st_poff[(size_t)g.pair_dst[p] + 1]++;
    for (int s = 0; s < S; ++s) st_poff[(size_t)s + 1] += st_poff[s];
    std::vector<int> fill(st_poff.begin(), st_poff.end() - 1), pair_at((size_t)P);
    for (int p = 0; p < P; ++p) pair_at[(size_t)fill[g.pair_dst[p]]++] = p;          // stp position -> pair
    int o = 0;
    for (int k = 0; k < P; ++k) {
        const int p = pair_at[k];
        stp[k] = int4{p, g.pair_lab[p], o, o + (int)g.in_arcs_of_pair[p].size()};
        for (auto &a : g.in_arcs_of_pair[p]) bt->farcs[(size_t)o++] = int2{a.first, (int)wbits(a.second)};
    }
    o = 0;
    for (int s = 0; s < S; ++s) {
        for (auto &a : g.out_arcs_of_state[s]) bt->barcs[(size_t)o++] = int2{a.first, (int)wbits(a.second)};
        bst_off[(size_t)s + 1] = o;
    }
    std::vector<int> ord((size_t)S);
    std::iota(ord.begin(), ord.end(), 0);
    auto fdeg = [&](int s) { return st_poff[(size_t)s + 1] > st_poff[s] ? stp[(size_t)st_poff[(size_t)s + 1] - 1].w - stp[(size_t)st_poff[s]].z : 0; };
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return fdeg(x) > fdeg(y); });
    for (int r = 0; r < S; ++r) {
        const int s0 = ord[(size_t)r], k0 = st_poff[s0], k1 = st_poff[(size_t)s0 + 1];
        bt->frow_d[(size_t)r] = s0;
        // one entering pair (every state of a T o LM graph): pair id and label sit in the descriptor itself
        bt->frow[(size_t)r] = k1 - k0 == 1 ? int4{stp[k0].z, stp[k0].w, stp[k0].x, stp[k0].y | 0x40000000}
                            : k1 > k0 ? int4{stp[k0].z, stp[(size_t)k1 - 1].w, k0, k1} : int4{0, 0, 0, 0};
    }
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return bst_off[(size_t)x + 1] - bst_off[x] > bst_off[(size_t)y + 1] - bst_off[y]; });
    for (int r = 0; r < S; ++r) {
        const int s0 = ord[(size_t)r];
        bt->brow_s[(size_t)r] = s0;
        const int k0 = st_poff[s0], k1 = st_poff[(size_t)s0 + 1];
        bt->brow[(size_t)r] = k1 - k0 == 1 ? int4{bst_off[s0], bst_off[(size_t)s0 + 1], stp[k0].x, stp[k0].y | 0x40000000}
                            : k1 > k0 ? int4{bst_off[s0], bst_off[(size_t)s0 + 1], k0, k1} : int4{bst_off[s0], bst_off[(size_t)s0 + 1], 0, 0};
    }
    for (int p = 0; p < P; ++p) bt->lab_off[(size_t)g.pair_lab[p] + 1]++;
    for (int v = 0; v <= g.max_label; ++v) bt->lab_off[(size_t)v + 1] += bt->lab_off[v];
}

// Factored rows of the utterance-minor kernels (crf_internal.h: StreamDev) from the BatchDev tables.  Structure detection as
// in the register-resident factored layout (res_layout.cpp build_factored), restated on these tables:
//   tail t, main o:  t has one entering pair whose two arcs come from t itself and from o with the same weight bits; both
//                    states have exactly one entering pair; a state is in at most one such couple;
//   forward rows:    every other one-pair row, the arcs from a couple's two states with equal weights merged into one record
//                    reading U = S + k; the main row carries its tail as second output;
//   backward rows:   a couple whose out-arcs are common except at most one each shares a row.
// Anything that does not fit stays what it was (one-pair rows: plain stream rows; the others: the row-at-a-time path).
// Used when at least half of the states are in couples.
static void build_batch_factored(int S, const BatchHost &bt, const std::vector<float> &start_lin, FacBatchH *fb) {
    const std::vector<int4> &frow = bt.frow, &brow = bt.brow;
    const std::vector<int> &frow_d = bt.frow_d, &brow_s = bt.brow_s;
    const std::vector<int2> &farcs = bt.farcs, &barcs = bt.barcs;
    FacBatchH &F = *fb;
    F = FacBatchH();
    if (opt_on(kOpt_bat_no_fac)) return;
    std::vector<int> fr_of(S, -1), br_of(S, -1);
    for (int r = 0; r < S; ++r) { fr_of[(size_t)frow_d[(size_t)r]] = r; br_of[(size_t)brow_s[(size_t)r]] = r; }
    auto fsimple = [&](int s) { const int4 &d = frow[(size_t)fr_of[(size_t)s]]; return (d.w & 0x40000000) && d.y > d.x; };
    auto bsimple = [&](int s) { const int4 &d = brow[(size_t)br_of[(size_t)s]]; return (d.w & 0x40000000) && d.y > d.x; };
    std::vector<int> main_of(S, -1), tail_of(S, -1), uidx(S, -1), tailw(S, 0);
    int NU = 0;
    for (int t = 0; t < S; ++t) {
        if (!fsimple(t)) continue;
        const int4 &d = frow[(size_t)fr_of[(size_t)t]];
        if (d.y - d.x != 2) continue;
        const int2 a = farcs[(size_t)d.x], b = farcs[(size_t)d.x + 1];
        if (a.y != b.y) continue;
        const int o = a.x == t ? b.x : b.x == t ? a.x : -1;
        if (o < 0 || o == t || !fsimple(o)) continue;
        if (main_of[(size_t)t] >= 0 || tail_of[(size_t)t] >= 0 || main_of[(size_t)o] >= 0 || tail_of[(size_t)o] >= 0) continue;
        main_of[(size_t)t] = o; tail_of[(size_t)o] = t; tailw[(size_t)o] = a.y;
    }
    // (a main state must not itself look like a tail that was skipped: nothing to check -- couples are disjoint by construction)
    for (int o = 0; o < S; ++o) if (tail_of[(size_t)o] >= 0) uidx[(size_t)o] = NU++;
    if ((int64_t)NU * 4 < S) return;
    auto couple_main = [&](int s) { return tail_of[(size_t)s] >= 0 ? s : main_of[(size_t)s]; };   // main state of s's couple, -1: none
    // forward
    for (int r = 0; r < S; ++r) {
        const int s = frow_d[(size_t)r];
        const int4 &d = frow[(size_t)r];
        if (!((d.w & 0x40000000) && d.y > d.x)) { F.frest.push_back(r); continue; }
        if (main_of[(size_t)s] >= 0) continue;                        // a tail: computed by its main row
        FacRowH row;
        row.st0 = s; row.pr0 = d.z; row.lab0 = d.w & 0xffff;
        if (tail_of[(size_t)s] >= 0) {
            const int t = tail_of[(size_t)s];
            const int4 &dt = frow[(size_t)fr_of[(size_t)t]];
            row.st1 = t; row.pr1 = dt.z; row.lab1 = dt.w & 0xffff; row.x0 = S + uidx[(size_t)s]; row.w0 = tailw[(size_t)s];
        }
        std::map<std::pair<int, int>, std::vector<int>> by;          // (couple's main, weight bits) -> arcs
        for (int k = d.x; k < d.y; ++k) by[{couple_main(farcs[(size_t)k].x), farcs[(size_t)k].y}].push_back(k);
        std::vector<char> used((size_t)(d.y - d.x), 0);
        for (int k = d.x; k < d.y; ++k) {
            if (used[(size_t)(k - d.x)]) continue;
            used[(size_t)(k - d.x)] = 1;
            const int src = farcs[(size_t)k].x, mn = couple_main(src);
            int partner = -1;
            if (mn >= 0) {
                const int other = src == mn ? tail_of[(size_t)mn] : mn;
                for (int q : by[{mn, farcs[(size_t)k].y}]) if (!used[(size_t)(q - d.x)] && farcs[(size_t)q].x == other) { partner = q; break; }
            }
            if (partner >= 0) { used[(size_t)(partner - d.x)] = 1; row.recs.push_back(int2{S + uidx[(size_t)mn], farcs[(size_t)k].y}); }
            else row.recs.push_back(farcs[(size_t)k]);
        }
        F.recs_f += (int64_t)row.recs.size();
        F.frows.push_back(std::move(row));
    }
    // backward
    std::vector<char> done(S, 0);
    for (int r = 0; r < S; ++r) {
        const int s = brow_s[(size_t)r];
        const int4 &d = brow[(size_t)r];
        if (!((d.w & 0x40000000) && d.y > d.x)) { F.brest.push_back(r); continue; }
        if (done[(size_t)s]) continue;
        done[(size_t)s] = 1;
        FacRowH row;
        row.st0 = s; row.pr0 = d.z; row.lab0 = d.w & 0xffff;
        const int mn = couple_main(s), m = mn < 0 ? -1 : (s == mn ? tail_of[(size_t)mn] : mn);
        bool fused = false;
        if (m >= 0 && !done[(size_t)m] && bsimple(m)) {
            const int4 &dm = brow[(size_t)br_of[(size_t)m]];
            std::vector<std::pair<int, int>> a, b, common, ea, eb;
            for (int k = d.x; k < d.y; ++k) a.push_back({barcs[(size_t)k].x, barcs[(size_t)k].y});
            for (int k = dm.x; k < dm.y; ++k) b.push_back({barcs[(size_t)k].x, barcs[(size_t)k].y});
            std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
            std::set_intersection(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(common));
            std::set_difference(a.begin(), a.end(), common.begin(), common.end(), std::back_inserter(ea));
            std::set_difference(b.begin(), b.end(), common.begin(), common.end(), std::back_inserter(eb));
            if (!common.empty() && ea.size() <= 1 && eb.size() <= 1) {
                fused = true;
                done[(size_t)m] = 1;
                row.st1 = m; row.pr1 = dm.z; row.lab1 = dm.w & 0xffff;
                if (!ea.empty()) { row.x0 = ea[0].first; row.w0 = ea[0].second; }
                if (!eb.empty()) { row.x1 = eb[0].first; row.w1 = eb[0].second; }
                for (auto &c : common) row.recs.push_back(int2{c.first, c.second});
            }
        }
        if (!fused) for (int k = d.x; k < d.y; ++k) row.recs.push_back(barcs[(size_t)k]);
        F.recs_b += (int64_t)row.recs.size();
        F.brows.push_back(std::move(row));
    }
    auto by_len = [](const FacRowH &x, const FacRowH &y) { return x.recs.size() > y.recs.size(); };
    std::stable_sort(F.frows.begin(), F.frows.end(), by_len);
    std::stable_sort(F.brows.begin(), F.brows.end(), by_len);
    F.x_start.assign((size_t)S + NU, 0.f);
    for (int s2 = 0; s2 < S; ++s2) {
        F.x_start[(size_t)s2] = start_lin[(size_t)s2];
        if (tail_of[(size_t)s2] >= 0) F.x_start[(size_t)S + uidx[(size_t)s2]] = start_lin[(size_t)s2] + start_lin[(size_t)tail_of[(size_t)s2]];
    }
    F.NU = NU;
    F.ok = 1;
}

void build_batch_tables(const PairGraph &g, BatchHost *bt, FacBatchH *fb) {
    build_batch_plain(g, bt);
    build_batch_factored(g.S, *bt, g.start_lin, fb);
}

// Host check of the factored rows (tests; no GPU): on random vectors, one step of both recursions through the factored rows
// (U entries, folded tail rows, fused backward rows) equals the step through the plain tables, pair by pair and state by
// state (fp64, 1e-12).  out: {NU, forward records, backward records, plain arcs}.
int debug_check_facbatch(const HostGraph *h, int64_t *out4) {
    const FacBatchH &F = h->fb;
    for (int i = 0; i < 4; ++i) out4[i] = 0;
    if (!F.ok) return CRF_OK;
    auto fl = [](int b) { float f; memcpy(&f, &b, 4); return (double)f; };
    const int S = (int)h->S, P = (int)h->P;
    uint64_t rng = 88172645463325252ull;
    auto rnd = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (double)(rng % 1000003) / 1000003.0 + 0.01; };
    std::vector<double> a((size_t)S), z((size_t)P), x((size_t)S + F.NU, 0.0);
    for (auto &v : a) v = rnd();
    for (auto &v : z) v = rnd();
    // U entries from the couples: found through the forward rows' second outputs
    for (int s = 0; s < S; ++s) x[(size_t)s] = a[(size_t)s];
    for (const FacRowH &r : F.frows) if (r.st1 >= 0) x[(size_t)r.x0] = a[(size_t)r.st0] + a[(size_t)r.st1];
    auto fail = [&](const char *why) { set_error(std::string("factored batch rows: ") + why); return CRF_ERR_ARG; };
    std::vector<double> q_plain((size_t)P, -1.0), q_fac((size_t)P, -1.0), b_plain((size_t)S, -1.0), b_fac((size_t)S, -1.0);
    std::vector<char> in_rest_f((size_t)S, 0), in_rest_b((size_t)S, 0);
    for (int r : F.frest) in_rest_f[(size_t)r] = 1;
    for (int r : F.brest) in_rest_b[(size_t)r] = 1;
    for (int r = 0; r < S; ++r) {
        const int4 &d = h->hb_frow[(size_t)r];
        if (in_rest_f[(size_t)r]) continue;
        double acc = 0.0;
        for (int k = d.x; k < d.y; ++k) acc += fl(h->hb_farcs[(size_t)k].y) * a[(size_t)h->hb_farcs[(size_t)k].x];
        q_plain[(size_t)d.z] = acc;
    }
    for (const FacRowH &r : F.frows) {
        double acc = 0.0;
        for (const int2 &c : r.recs) acc += fl(c.y) * x[(size_t)c.x];
        if (q_fac[(size_t)r.pr0] >= 0.0) return fail("a pair is produced twice (forward)");
        q_fac[(size_t)r.pr0] = acc;
        if (r.st1 >= 0) { if (q_fac[(size_t)r.pr1] >= 0.0) return fail("a pair is produced twice (forward, tail)"); q_fac[(size_t)r.pr1] = fl(r.w0) * x[(size_t)r.x0]; }
    }
    for (int p2 = 0; p2 < P; ++p2) {
        if ((q_plain[(size_t)p2] < 0.0) != (q_fac[(size_t)p2] < 0.0)) return fail("forward rows do not cover the one-pair rows");
        if (q_plain[(size_t)p2] >= 0.0 && std::fabs(q_plain[(size_t)p2] - q_fac[(size_t)p2]) > 1e-9 * std::fabs(q_plain[(size_t)p2])) return fail("a forward row's sum differs");
    }
    for (int r = 0; r < S; ++r) {
        const int4 &d = h->hb_brow[(size_t)r];
        if (in_rest_b[(size_t)r]) continue;
        double acc = 0.0;
        for (int k = d.x; k < d.y; ++k) acc += fl(h->hb_barcs[(size_t)k].y) * z[(size_t)h->hb_barcs[(size_t)k].x];
        b_plain[(size_t)h->hb_brow_s[(size_t)r]] = acc;
    }
    for (const FacRowH &r : F.brows) {
        double acc = 0.0;
        for (const int2 &c : r.recs) acc += fl(c.y) * z[(size_t)c.x];
        if (b_fac[(size_t)r.st0] >= 0.0) return fail("a state is produced twice (backward)");
        b_fac[(size_t)r.st0] = acc + fl(r.w0) * z[(size_t)r.x0];
        if (r.st1 >= 0) { if (b_fac[(size_t)r.st1] >= 0.0) return fail("a state is produced twice (backward, mate)"); b_fac[(size_t)r.st1] = acc + fl(r.w1) * z[(size_t)r.x1]; }
    }
    for (int s = 0; s < S; ++s) {
        if ((b_plain[(size_t)s] < 0.0) != (b_fac[(size_t)s] < 0.0)) return fail("backward rows do not cover the one-pair rows");
        if (b_plain[(size_t)s] >= 0.0 && std::fabs(b_plain[(size_t)s] - b_fac[(size_t)s]) > 1e-9 * std::fabs(b_plain[(size_t)s])) return fail("a backward row's sum differs");
    }
    // descriptors: pairs and labels as in the plain tables
    std::vector<int> fr_of((size_t)S, -1), br_of((size_t)S, -1);
    for (int r = 0; r < S; ++r) { fr_of[(size_t)h->hb_frow_d[(size_t)r]] = r; br_of[(size_t)h->hb_brow_s[(size_t)r]] = r; }
    auto desc_ok = [&](const std::vector<int4> &rows, const std::vector<int> &of, int st, int pr, int lab) {
        const int4 &d = rows[(size_t)of[(size_t)st]];
        return (d.w & 0x40000000) && d.z == pr && (d.w & 0xffff) == lab;
    };
    for (const FacRowH &r : F.frows) if (!desc_ok(h->hb_frow, fr_of, r.st0, r.pr0, r.lab0) || (r.st1 >= 0 && !desc_ok(h->hb_frow, fr_of, r.st1, r.pr1, r.lab1))) return fail("forward descriptor");
    for (const FacRowH &r : F.brows) if (!desc_ok(h->hb_brow, br_of, r.st0, r.pr0, r.lab0) || (r.st1 >= 0 && !desc_ok(h->hb_brow, br_of, r.st1, r.pr1, r.lab1))) return fail("backward descriptor");
    out4[0] = F.NU; out4[1] = F.recs_f; out4[2] = F.recs_b; out4[3] = h->A;
    return CRF_OK;
}

// steps per task: the longer direction's steps (rows padded to whole batches) over the tasks wanted; the switch bat_task overrides
static int stream_task_steps(const HostGraph *h, int AL, int want, bool fac = false) {
    constexpr int kB = kStreamBatch;
    const int epi = kBatEpiDefault * kB;   // (build_stream_rows: what a bundle's row epilogues cost, in steps)
    auto steps_of = [&](const std::vector<int4> &rows) {
        int64_t n = 0;
        for (const int4 &d : rows) if ((d.w & 0x40000000) && d.y > d.x) n += (d.y - d.x + kB - 1) / kB * kB + epi;
        return (n + AL - 1) / AL;                         // (rows of a bundle have about the same length)
    };
    auto steps_fac = [&](const std::vector<FacRowH> &rows) {
        int64_t n = 0;
        for (const FacRowH &r : rows) n += ((int64_t)r.recs.size() + kB - 1) / kB * kB + epi;
        return (n + AL - 1) / AL;
    };
    const int64_t steps = fac ? std::max(steps_fac(h->fb.frows), steps_fac(h->fb.brows)) : std::max(steps_of(h->hb_frow), steps_of(h->hb_brow));
    int task_steps = (int)std::min<int64_t>(4096, std::max<int64_t>(64, ((steps + want - 1) / want + kB - 1) / kB * kB));
    if (opt(kOpt_bat_task, 0) > 0) task_steps = std::max(8, opt(kOpt_bat_task, 0));
    return task_steps;
}

int debug_check_decode(int nslot, int ncombo) {
    if (nslot < 1 || ncombo < 1) { set_error("debug_check_decode: bad arguments"); return CRF_ERR_ARG; }
    std::map<std::pair<int, int>, int> seen;
    std::vector<int> nch((size_t)ncombo, -1);
    for (int b = 0; b < 8 * nslot; ++b) {
        int combo, chunk, nchunk;
        bat_decode(b, 8 * nslot, ncombo, &combo, &chunk, &nchunk);
        if (combo < 0 || combo >= ncombo) continue;      // (more XCDs than combos' residues can fill: a block without work)
        if (chunk < 0 || chunk >= nchunk) { set_error("bat_decode: chunk out of range"); return CRF_ERR_ARG; }
        if (nch[(size_t)combo] >= 0 && nch[(size_t)combo] != nchunk) { set_error("bat_decode: blocks of a combo disagree on its chunk count"); return CRF_ERR_ARG; }
        nch[(size_t)combo] = nchunk;
        if (seen[{combo, chunk}]++) { set_error("bat_decode: a (combo, chunk) is taken twice"); return CRF_ERR_ARG; }
    }
    for (int c = 0; c < ncombo; ++c) {
        if (nch[(size_t)c] < 1) { set_error("bat_decode: a combo has no workgroup"); return CRF_ERR_ARG; }
        for (int k = 0; k < nch[(size_t)c]; ++k) if (!seen.count({c, k})) { set_error("bat_decode: a chunk of a combo is missing"); return CRF_ERR_ARG; }
    }
    return CRF_OK;
}

// Structure check of a stream against the rows it was cut from (any descriptor width): bundle i holds rows [i * AL, (i + 1) * AL)
// in order, records = the row's records (entry * UL) followed by null records up to the bundle's whole batches, the end flag in
// the first record of the bundle's last batch for every lane group and nowhere else, descriptors word for word, a task has
// at most maxb bundles and the tasks cover the bundles in order.  out: {tasks, 0, steps, records that are not padding}.
static int check_stream_rows(int AL, int UL, int NM, int maxb, const StreamHost &sh, const std::vector<SRow> &srows, int64_t *out) {
    constexpr int kB = kStreamBatch;
    auto fail = [&](const char *why) { set_error(std::string("arc stream check (rows): ") + why); return CRF_ERR_ARG; };
    int next_bundle = 0;
    int64_t steps = 0, real = 0;
    for (const int4 &t : sh.tasks) {
        if (t.w < 1 || t.w > maxb) return fail("a task has no or too many bundles");
        if (t.z != next_bundle) return fail("the tasks do not cover the bundles in order");
        next_bundle += t.w;
        int batch = t.x;
        for (int b = 0; b < t.w; ++b) {
            int nbat = 0;
            for (;;) {
                if (batch + nbat >= t.x + t.y) return fail("a bundle runs past its task");
                const int2 first = sh.recs[((size_t)(batch + nbat) * AL + 0) * kB];
                ++nbat;
                if (first.x < 0) break;
            }
            for (int aj = 0; aj < AL; ++aj) {
                const int i = (t.z + b) * AL + aj;
                const bool have = i < (int)srows.size();
                for (int q = 0; q < NM; ++q) {
                    const int4 m = sh.meta[((size_t)(t.z + b) * AL + aj) * NM + q], w = have ? srows[(size_t)i].m[q] : int4{-1, 0, 0, 0};
                    if (m.x != w.x || m.y != w.y || m.z != w.z || m.w != w.w) return fail("a descriptor word");
                }
                const int n = have ? srows[(size_t)i].n : 0;
                if (n > nbat * kB) return fail("a row is longer than its bundle");
                for (int st = 0; st < nbat * kB; ++st) {
                    const int2 rc = sh.recs[((size_t)(batch + st / kB) * AL + aj) * kB + st % kB];
                    if ((rc.x < 0) != (st == (nbat - 1) * kB)) return fail("end-of-bundle flag");
                    const int idx = rc.x & 0x7fffffff;
                    if (st < n) {
                        if (idx != srows[(size_t)i].recs[st].x * UL || rc.y != srows[(size_t)i].recs[st].y) return fail("a record is not its row's");
                        ++real;
                    } else if (idx != 0 || rc.y != 0) return fail("padding record is not null");
                }
            }
            batch += nbat; steps += (int64_t)nbat * kB;
        }
        if (batch != t.x + t.y) return fail("batches of a task");
    }
    if (next_bundle != ((int)srows.size() + AL - 1) / AL) return fail("bundles missing");
    out[0] += (int64_t)sh.tasks.size(); out[2] += steps; out[3] += real;
    return CRF_OK;
}

// Builds the arc streams of both directions on the host and checks them (check_stream_host); no device needed.
int debug_check_streams(const HostGraph *h, int UL, int want, int64_t *out4) {
    const bool fac = UL < 0;                             // -UL: the factored streams (graphs with factored rows)
    if (fac) UL = -UL;
    if (!h || !(UL == 8 || UL == 16 || UL == 32 || UL == 64) || want < 1 || !out4) { set_error("debug_check_streams: bad arguments"); return CRF_ERR_ARG; }
    const int AL = 256 / UL, task_steps = stream_task_steps(h, AL, want, fac);
    for (int i = 0; i < 4; ++i) out4[i] = 0;
    if (fac) {
        if (!h->fb.ok) return CRF_OK;
        for (int dir = 0; dir < 2; ++dir) {
            const std::vector<FacRowH> &rows = dir == 0 ? h->fb.frows : h->fb.brows;
            StreamHost sh;
            int rc = build_stream_host_fac(AL, UL, task_steps, rows, dir == 0 ? h->fb.frest : h->fb.brest, &sh);
            if (!rc) rc = check_stream_rows(AL, UL, 3, stream_max_bundles(UL, true), sh, fac_stream_rows(rows), out4);
            if (rc) return rc;
            out4[1] += (int64_t)sh.rest.size();
        }
        return CRF_OK;
    }
    for (int dir = 0; dir < 2; ++dir) {
        const std::vector<int4> &rows = dir == 0 ? h->hb_frow : h->hb_brow;
        const std::vector<int> &st = dir == 0 ? h->hb_frow_d : h->hb_brow_s;
        const std::vector<int2> &arcs = dir == 0 ? h->hb_farcs : h->hb_barcs;
        StreamHost sh;
        int rc = build_stream_host(AL, UL, task_steps, rows, st, arcs, &sh);
        if (!rc) rc = check_stream_host(AL, UL, sh, rows, st, arcs, out4);
        if (rc) return rc;
    }
    return CRF_OK;
}

bool stream_fac(const HostGraph *h, int UL) { (void)UL; return h && h->fb.ok && !opt_on(kOpt_bat_no_fac); }

int ensure_stream_tables(HostGraph *h, int UL, int want, const StreamDev **out) {
    const int AL = 256 / std::max(UL, 1);                 // lane groups: a lane takes 4 utterances, UL / 4 lanes a row
    static std::mutex mu;
    if (!h || !(UL == 8 || UL == 16 || UL == 32 || UL == 64) || want < 1 || !h->dev.bat.ok) { set_error("ensure_stream_tables: bad arguments"); return CRF_ERR_ARG; }
    std::lock_guard<std::mutex> lock(mu);
    const bool fac = stream_fac(h, UL);
    for (StreamDev *sd : h->streams)
        if (sd->AL == AL && sd->want == want && (sd->fac != 0) == fac) { *out = sd; return CRF_OK; }
    // factored streams for T o LM graphs
    const int task_steps = stream_task_steps(h, AL, want, fac);
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(h->device) != hipSuccess) { set_error("ensure_stream_tables: cannot select the graph's device"); return CRF_ERR_HIP; }
    auto *sd = new StreamDev();
    int rc = CRF_OK;
    for (int dir = 0; dir < 2 && !rc; ++dir) {
        StreamHost sh;
        if (fac) rc = build_stream_host_fac(AL, UL, task_steps, dir == 0 ? h->fb.frows : h->fb.brows, dir == 0 ? h->fb.frest : h->fb.brest, &sh);
        else rc = dir == 0 ? build_stream_host(AL, UL, task_steps, h->hb_frow, h->hb_frow_d, h->hb_farcs, &sh)
                           : build_stream_host(AL, UL, task_steps, h->hb_brow, h->hb_brow_s, h->hb_barcs, &sh);
        if (!rc) rc = upload_stream(h, sh, dir == 0 ? &sd->f : &sd->b);
    }
    sd->fac = fac ? 1 : 0; sd->NU = fac ? h->fb.NU : 0;
    if (fac) { if (!rc) rc = upload(h, h->fb.x_start, &sd->x_start); }
    else sd->x_start = h->dev.start_lin;
    (void)hipSetDevice(prev);
    if (rc) { delete sd; return rc; }
    sd->AL = AL; sd->want = want; sd->ok = 1;
    h->streams.push_back(sd);
    *out = sd;
    return CRF_OK;
}

}  // namespace crf

extern "C" {

int crf_debug_decode_check(int nslot, int ncombo) { return crf::debug_check_decode(nslot, ncombo); }

int crf_debug_facbatch_check(const crf_graph *g, int64_t *out4) {
    if (!g || !g->h || !out4) { crf::set_error("null argument"); return CRF_ERR_ARG; }
    return crf::debug_check_facbatch(g->h, out4);
}

int crf_debug_stream_check(const crf_graph *g, int UL, int want, int64_t *out4) {
    if (!g || !g->h) { crf::set_error("null graph"); return CRF_ERR_ARG; }
    return crf::debug_check_streams(g->h, UL, want, out4);
}

}  // extern "C"
