#include "multi_gpu.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <thread>

namespace mkhost {

std::vector<int> device_list()
{
    std::vector<int> out;
    if (const char *e = getenv("MIEKKI_DEVICES")) {
        const char *p = e;
        while (*p) {
            char *end = nullptr;
            const long v = strtol(p, &end, 10);
            if (end == p) break;
            out.push_back((int)v);
            p = *end == ',' ? end + 1 : end;
        }
        if (!out.empty()) return out;
    }
    if (const char *e = getenv("MIEKKI_DEVICE")) return {atoi(e)};          // one GPU, by ordinal
    const int n = mk_device_count();
    for (int d = 0; d < n; ++d) out.push_back(d);
    if (out.empty()) out.push_back(0);                                       // mk_create will say why it fails
    return out;
}

DeviceGroup::~DeviceGroup()
{
    if (!ctx_.empty()) {
        for (size_t d = 1; d < d_rows_.size(); ++d) mk_dev_free(ctx_[d], d_rows_[d]);
        mk_dev_free(ctx_[0], d_gather_);
        mk_dev_free(ctx_[0], d_hits_);
        mk_dev_free(ctx_[0], d_nhits_);
    }
    if (comm_) mk_comm_destroy(comm_);
    for (mk_ctx *c : ctx_) mk_destroy(c);
}

uint32_t DeviceGroup::total() const
{
    if (!base_.empty()) return base_.back();
    uint32_t n = 0;
    for (mk_ctx *c : ctx_) n += mk_index_size(c);
    return n;
}

size_t DeviceGroup::owner(uint32_t genome) const
{
    size_t d = 0;
    while (d + 1 < ctx_.size() && genome >= base_[d + 1]) ++d;
    return d;
}

int DeviceGroup::finish(bool merge_bloom, std::string &err)
{
    if (comm_) {
        // one process per GPU: the Bloom fold is a MIN all-reduce over rank-keyed cells, the id bases and the sizes of
        // all genomes come from two all-gathers (mk_comm_share_sizes hands them to the merge as well)
        uint32_t base = 0, total = 0;
        if ((merge_bloom && mk_comm_sync_bloom(comm_) != MK_OK) || mk_comm_share_sizes(comm_, &base, &total) != MK_OK) { err = mk_last_error(); return -1; }
        my_base_ = base;
        base_.assign({0u, total});
        gs_all_.assign(total, 0);
        ss_all_.assign(total, 0);
        if (total && mk_merge_get_sizes(ctx_[0], gs_all_.data(), ss_all_.data(), total) != MK_OK) { err = mk_last_error(); return -1; }
        any_empty_sketch_ = false;
        for (uint32_t v : ss_all_) any_empty_sketch_ |= v == 0;
        const uint32_t mine = mk_index_size(ctx_[0]);
        std::vector<uint8_t> all;
        if (all_gather_bytes(&mine, 4, all, err)) return -1;
        largest_shard_ = 0;
        for (int r = 0; r < world(); ++r) { uint32_t n; memcpy(&n, all.data() + 4 * r, 4); largest_shard_ = std::max(largest_shard_, n); }
        return 0;
    }
    const size_t D = ctx_.size();
    base_.assign(D + 1, 0);
    for (size_t d = 0; d < D; ++d) {
        base_[d + 1] = base_[d] + mk_index_size(ctx_[d]);
        if (mk_set_genome_id_base(ctx_[d], base_[d]) != MK_OK) { err = mk_last_error(); return -1; }
    }
    gs_all_.assign(base_[D], 0);
    ss_all_.assign(base_[D], 0);
    for (size_t d = 0; d < D; ++d)
        if (mk_index_export_sizes(ctx_[d], gs_all_.data() + base_[d], ss_all_.data() + base_[d]) != MK_OK) {
            err = mk_last_error();
            return -1;
        }
    if (D == 1) return 0;
    if (mk_merge_set_sizes(ctx_[0], gs_all_.data(), ss_all_.data(), base_[D], 0) != MK_OK) { err = mk_last_error(); return -1; }
    const uint64_t reach = mk_bloom_reachable_bytes(ctx_[0]);
    if (!merge_bloom || !reach) return 0;
    // fold the shards' filters in shard order on the first shard's GPU, then hand the result back
    void *stage = nullptr;
    std::vector<void *> buf(D, nullptr);
    int rc = 0;
    auto fail = [&]() { err = mk_last_error(); rc = -1; };
    if (mk_dev_alloc(ctx_[0], reach, &stage) != MK_OK) fail();
    for (size_t d = 1; d < D && !rc; ++d) {
        if (mk_dev_alloc(ctx_[d], reach, &buf[d]) != MK_OK) { fail(); break; }
        if (mk_index_export_bloom_device(ctx_[d], 0, reach, (uint8_t *)buf[d]) != MK_OK ||
            mk_dev_copy(ctx_[0], stage, ctx_[d], buf[d], reach) != MK_OK ||
            mk_index_merge_bloom_device(ctx_[0], 0, reach, (const uint8_t *)stage) != MK_OK)
            fail();
    }
    if (!rc && mk_index_export_bloom_device(ctx_[0], 0, reach, (uint8_t *)stage) != MK_OK) fail();
    for (size_t d = 1; d < D && !rc; ++d)
        if (mk_dev_copy(ctx_[d], buf[d], ctx_[0], stage, reach) != MK_OK ||
            mk_index_import_bloom_device(ctx_[d], 0, reach, (const uint8_t *)buf[d]) != MK_OK)
            fail();
    for (size_t d = 1; d < D; ++d) mk_dev_free(ctx_[d], buf[d]);
    mk_dev_free(ctx_[0], stage);
    return rc;
}

int DeviceGroup::select(const uint32_t *ids, uint32_t n, std::string &err)
{
    if (comm_) { err = "selecting genomes is not supported with one process per GPU"; return -1; }
    if (!n) { err = "no genome ids"; return -1; }
    const size_t D = ctx_.size();
    if (D > 1 && !std::is_sorted(ids, ids + n)) { err = "a list that is not ascending would move genomes between GPUs"; return -1; }
    // the query buffers were sized for the old shards (none exist before the first query)
    for (size_t d = 1; d < d_rows_.size(); ++d) mk_dev_free(ctx_[d], d_rows_[d]);
    if (!d_rows_.empty() || d_gather_) { mk_dev_free(ctx_[0], d_gather_); mk_dev_free(ctx_[0], d_hits_); mk_dev_free(ctx_[0], d_nhits_); }
    d_rows_.clear();
    d_gather_ = d_hits_ = d_nhits_ = nullptr;
    rows_cap_ = hits_cap_ = nhits_cap_ = 0;
    std::vector<mk_ctx *> kept;
    uint32_t j = 0;
    for (size_t d = 0; d < D; ++d) {
        uint32_t e = j;
        while (D > 1 && e < n && ids[e] < base_[d + 1]) ++e;          // (ascending: shard d's ids are a run of the list)
        if (D == 1) e = n;
        if (e == j) { mk_destroy(ctx_[d]); continue; }               // nothing of this shard stays
        if (mk_index_select(ctx_[d], ids + j, e - j) != MK_OK) {
            err = mk_last_error();
            kept.insert(kept.end(), ctx_.begin() + d, ctx_.end());
            ctx_.swap(kept);
            return -1;
        }
        kept.push_back(ctx_[d]);
        j = e;
    }
    ctx_.swap(kept);
    return finish(false, err);
}

int DeviceGroup::extend(mk_ctx *src, std::string &err)
{
    if (comm_ || ctx_.size() != 1) { err = "joining indexes takes one GPU in one process"; return -1; }
    if (mk_index_extend(ctx_[0], src) != MK_OK) { err = mk_last_error(); return -1; }
    return finish(false, err);
}

// One thread per shard: f(d) -> an MK_* code, all joined.  0, or -1 with err = the message of the first shard that failed.
// A shard that answers MK_ERR_UNSUPPORTED (the NaN corner) has not failed when the caller asks about it: *unsupported.
template <typename F>
static int on_shards(size_t D, std::string &err, bool *unsupported, F f)
{
    std::vector<int> rc(D, MK_OK);
    std::vector<std::string> msg(D);
    std::vector<std::thread> th;
    for (size_t d = 0; d < D; ++d)
        th.emplace_back([&, d] {
            rc[d] = f(d);
            if (rc[d] != MK_OK) msg[d] = mk_last_error();
        });
    for (auto &t : th) t.join();
    if (unsupported) *unsupported = false;
    for (size_t d = 0; d < D; ++d) {
        if (unsupported && rc[d] == MK_ERR_UNSUPPORTED) *unsupported = true;
        else if (rc[d] != MK_OK) { err = msg[d]; return -1; }
    }
    return 0;
}

// entrant slots per query of a shard's exchange row: the largest shard decides the row width
uint32_t DeviceGroup::row_cap(uint32_t nresults) const
{
    uint64_t largest = largest_shard_;                                // (ranked: the shards are other processes')
    for (size_t d = 0; !comm_ && d + 1 < base_.size(); ++d) largest = std::max<uint64_t>(largest, base_[d + 1] - base_[d]);
    return std::min(entrant_cap(nresults, largest), kCapWide);
}

int DeviceGroup::ensure_buffers(uint32_t nq, uint32_t nresults, uint32_t cap, std::string &err)
{
    const size_t D = ctx_.size();
    const uint64_t words = (uint64_t)std::max<uint64_t>(nq, 1024) * (cap + 1);      // 8-byte row words per shard
    if (words > rows_cap_) {
        for (size_t d = 1; d < d_rows_.size(); ++d) mk_dev_free(ctx_[d], d_rows_[d]);
        mk_dev_free(ctx_[0], d_gather_);
        d_rows_.assign(D, nullptr);
        d_gather_ = nullptr;
        rows_cap_ = 0;
        if (mk_dev_alloc(ctx_[0], D * words * 8, &d_gather_) != MK_OK) { err = mk_last_error(); return -1; }
        for (size_t d = 1; d < D; ++d)
            if (mk_dev_alloc(ctx_[d], words * 8, &d_rows_[d]) != MK_OK) {
                // leave nothing half-made behind: the next call starts from empty buffers
                err = mk_last_error();
                for (size_t e = 1; e < D; ++e) { mk_dev_free(ctx_[e], d_rows_[e]); d_rows_[e] = nullptr; }
                mk_dev_free(ctx_[0], d_gather_);
                d_gather_ = nullptr;
                return -1;
            }
        rows_cap_ = words;
    }
    const uint64_t need_nh = std::max<uint64_t>(nq, 1024);
    if (need_nh > nhits_cap_) {
        mk_dev_free(ctx_[0], d_nhits_);
        d_nhits_ = nullptr; nhits_cap_ = 0;
        if (mk_dev_alloc(ctx_[0], need_nh * 4, &d_nhits_) != MK_OK) { err = mk_last_error(); return -1; }
        nhits_cap_ = need_nh;
    }
    const uint64_t need_hits = need_nh * std::max(nresults, 1u);
    if (need_hits > hits_cap_) {
        mk_dev_free(ctx_[0], d_hits_);
        d_hits_ = nullptr; hits_cap_ = 0;
        if (mk_dev_alloc(ctx_[0], need_hits * sizeof(mk_hit), &d_hits_) != MK_OK) { err = mk_last_error(); return -1; }
        hits_cap_ = need_hits;
    }
    return 0;
}

int DeviceGroup::query(const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t nresults, uint32_t min_score,
                       double min_inter, mk_hit *hits, uint32_t *nhits, std::string &err)
{
    if (ctx_.size() == 1 && !comm_) {
        if (mk_query(ctx_[0], seqs, lens, nq, nresults, min_score, min_inter, hits, nhits, nullptr) != MK_OK) {
            err = mk_last_error();
            return -1;
        }
        return 0;
    }
    if (!nq) return 0;
    std::vector<uint32_t> all(nq);                                    // (mk_qset_upload handles mixed sets)
    std::iota(all.begin(), all.end(), 0u);
    const uint32_t cap = row_cap(nresults);
    if (comm_) {
        // NaN corner (min_score 0 over an index that holds an empty sketch ANYWHERE: every rank decides alike) and
        // top-N sizes beyond the device selection: dense score rows of every rank
        if (nresults > 64 || (min_score == 0 && any_empty_sketch_))
            return replay_ranked(all, seqs, lens, nresults, min_score, min_inter, hits, nhits, err);
        return query_ranked(all, seqs, lens, nresults, min_score, min_inter, hits, nhits, cap, err);
    }
    const Queries qy{seqs, lens, nullptr};
    if (nresults > 64) return replay(qy, all, nullptr, nresults, min_score, min_inter, hits, nhits, err);
    return sharded_pass(qy, all, nresults, min_score, min_inter, hits, nhits, cap, err);
}

static void merge_candidate_lists(const std::vector<mk_hitlist *> &lists, uint32_t nq, uint32_t nresults, uint32_t q0,
                                  std::vector<uint64_t> &offsets, std::vector<mk_hit> &hits);

// The lists of nq queries from every shard -- run(d, &list) -- as ONE list per query, queries q0 .. of `offsets`, their hits
// appended to `hits`.  One shard: ordered on the device already.  Several: one heap over the shards' candidates.
template <typename Run>
int DeviceGroup::merged_lists(uint32_t nq, uint32_t nresults, uint32_t q0, Run run, std::vector<uint64_t> &offsets, std::vector<mk_hit> &hits,
                              std::string &err)
{
    const size_t D = ctx_.size();
    std::vector<mk_hitlist *> lists(D, nullptr);
    const int ret = on_shards(D, err, nullptr, [&](size_t d) { return run(d, &lists[d]); });
    if (ret == 0 && D == 1) {
        const uint64_t *off = mk_hitlist_offsets(lists[0]);
        const mk_hit *h = mk_hitlist_hits(lists[0]);
        const uint64_t at = hits.size();
        hits.insert(hits.end(), h, h + off[nq]);
        for (uint32_t q = 0; q < nq; ++q) offsets[q0 + q + 1] = at + off[q + 1];
    } else if (ret == 0) {
        merge_candidate_lists(lists, nq, nresults, q0, offsets, hits);
    }
    for (mk_hitlist *l : lists) mk_hitlist_free(l);
    return ret;
}

int DeviceGroup::query_list(const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t nresults, uint32_t min_score,
                            double min_inter, std::vector<uint64_t> &offsets, std::vector<mk_hit> &hits, std::string &err)
{
    offsets.assign((size_t)nq + 1, 0);
    hits.clear();
    if (comm_) { err = "lists of more than the reference's ten genomes are not exchanged between processes"; return -1; }
    const uint32_t per_shard = ctx_.size() == 1 ? nresults : MK_LIST_CANDIDATES;
    return merged_lists(nq, nresults, 0, [&](size_t d, mk_hitlist **out) {
        return mk_query_list(ctx_[d], seqs, lens, nq, per_shard, min_score, min_inter, out, nullptr);
    }, offsets, hits, err);
}

// every shard's query set of queries idx[0 .. n) of a call (free_sets releases them): uploaded sequences (mk_qset_upload
// handles mixed sets), or indexed genomes that ONE shard owns (indexed_sets)
int DeviceGroup::make_sets(const Queries &qy, const uint32_t *idx, uint32_t n, std::vector<mk_qset *> &sets, std::string &err)
{
    if (qy.ids) {
        std::vector<uint32_t> ids(n);
        for (uint32_t i = 0; i < n; ++i) ids[i] = qy.ids[idx[i]];
        return indexed_sets(ids.data(), n, sets, err);
    }
    std::vector<const char *> s(n);
    std::vector<uint64_t> l(n);
    for (uint32_t i = 0; i < n; ++i) { s[i] = qy.seqs[idx[i]]; l[i] = qy.lens[idx[i]]; }
    sets.assign(ctx_.size(), nullptr);
    if (on_shards(ctx_.size(), err, nullptr, [&](size_t d) { return mk_qset_upload(ctx_[d], s.data(), l.data(), n, &sets[d]); })) {
        free_sets(sets);
        return -1;
    }
    return 0;
}

// One pass over the shards for queries idx[] of a call (query i's hits go to place idx[i]): every shard's entrant rows, the
// one exchange step, the merge on the first GPU; rows that overflowed once more with wide rows; then dense score rows.
int DeviceGroup::sharded_pass(const Queries &qy, const std::vector<uint32_t> &idx, uint32_t nresults, uint32_t min_score, double min_inter,
                              mk_hit *hits, uint32_t *nhits, uint32_t cap, std::string &err)
{
    const size_t D = ctx_.size();
    const uint32_t n = (uint32_t)idx.size();
    if (ensure_buffers(n, nresults, cap, err)) return -1;
    std::vector<mk_qset *> sets;
    if (make_sets(qy, idx.data(), n, sets, err)) return -1;
    const uint64_t part_bytes = (uint64_t)n * (cap + 1) * 8;
    bool unsupported = false;                                         // NaN corner: answered from dense rows
    int r = on_shards(D, err, &unsupported, [&](size_t d) {
        // shard 0 writes straight into its slot of the gather buffer
        uint64_t *rows = d == 0 ? (uint64_t *)d_gather_ : (uint64_t *)d_rows_[d];
        int rc = mk_qset_run_compact(ctx_[d], sets[d], nresults, min_score, min_inter, cap, rows);
        // the ONE exchange step: this shard's entrant rows -> the merging GPU (peer DMA over xGMI)
        if (rc == MK_OK && d != 0) rc = mk_dev_copy(ctx_[0], (uint8_t *)d_gather_ + d * part_bytes, ctx_[d], rows, part_bytes);
        return rc == MK_OK ? mk_sync(ctx_[d]) : rc;
    });
    if (r == 0 && unsupported) r = replay(qy, idx, &sets, nresults, min_score, min_inter, hits, nhits, err);
    if (r || unsupported) { free_sets(sets); return r; }
    gather_bytes_ += (D - 1) * part_bytes;
    std::vector<uint32_t> nh(n);
    std::vector<mk_hit> hh((size_t)n * std::max(nresults, 1u));
    if (mk_merge_compact(ctx_[0], (const uint64_t *)d_gather_, (uint32_t)D, n, cap, nresults, (mk_hit *)d_hits_, (uint32_t *)d_nhits_) != MK_OK ||
        mk_dev_download(ctx_[0], nh.data(), d_nhits_, (uint64_t)n * 4) != MK_OK ||
        (nresults && mk_dev_download(ctx_[0], hh.data(), d_hits_, (uint64_t)n * nresults * sizeof(mk_hit)) != MK_OK)) {
        err = mk_last_error();
        free_sets(sets);
        return -1;
    }
    std::vector<uint32_t> over;
    for (uint32_t i = 0; i < n; ++i) {
        if (nh[i] == MK_MERGE_OVERFLOW) { over.push_back(idx[i]); continue; }
        nhits[idx[i]] = nh[i];
        std::copy(hh.begin() + (size_t)i * nresults, hh.begin() + (size_t)i * nresults + nh[i], hits + (size_t)idx[i] * nresults);
    }
    // More entrants than a row holds on some shard (tie-heavy collections: every copy of a genome is an
    // entrant).  Such queries run once more with wide rows -- still 8 bytes per entrant, still one exchange
    // step -- before anything falls back to dense score rows of every shard, which cost n x G words per
    // shard and the host's heap.  MIEKKI_SHARD_WIDE_ROWS=0 skips the second pass (the tests use it to keep
    // the dense replay covered).
    static const bool wide = [] { const char *e = getenv("MIEKKI_SHARD_WIDE_ROWS"); return !e || atoi(e) != 0; }();
    if (!over.empty() && wide && cap < kCapWide) {
        free_sets(sets);
        rerun_queries_ += over.size();
        for (size_t i0 = 0; i0 < over.size(); i0 += 4096) {           // bounded buffers: 4096 x 4097 x 8 B = 134 MB per shard
            const std::vector<uint32_t> piece(over.begin() + i0, over.begin() + std::min(over.size(), i0 + 4096));
            if (sharded_pass(qy, piece, nresults, min_score, min_inter, hits, nhits, kCapWide, err)) return -1;
        }
        return 0;
    }
    // (the sets serve the replay when it is of all their queries)
    if (!over.empty()) r = replay(qy, over, over.size() == n ? &sets : nullptr, nresults, min_score, min_inter, hits, nhits, err);
    free_sets(sets);
    return r;
}

// the reference's loop and heap (Miekki.cpp:376-397 as written) over complete score rows: sc[d] = shard d's rows of n
// queries; query i's hits go to where[i]
void DeviceGroup::filter_score_rows(const std::vector<std::vector<uint32_t>> &sc, uint32_t n, const uint32_t *where, uint32_t nresults,
                                    uint32_t min_score, double min_inter, mk_hit *hits, uint32_t *nhits) const
{
    const size_t D = ctx_.size();
    std::vector<mk_hit> full;
    for (uint32_t i = 0; i < n; ++i) {
        full.clear();
        for (size_t d = 0; d < D; ++d) {
            const uint32_t Gd = base_[d + 1] - base_[d];
            const uint32_t *row = sc[d].data() + (size_t)i * Gd;
            for (uint32_t g = 0; g < Gd; ++g) {
                if (row[g] < min_score) continue;
                const uint32_t id = base_[d] + g;
                const double jac = (double)row[g] / ss_all_[id];
                const double inter = jac * gs_all_[id];
                if (inter < min_inter) continue;
                full.push_back(mk_hit{id, row[g], jac, inter});
            }
        }
        const uint32_t q = where[i];
        nhits[q] = mk_filter_candidates(full.data(), (uint32_t)full.size(), nresults, hits + (size_t)q * nresults);
    }
}

// One heap (mk_filter_candidates) per query over the shards' candidate lists concatenated in shard order -- genome order:
// queries 0 .. nq of the lists are queries q0 .. of `offsets`, their hits appended to `hits`
static void merge_candidate_lists(const std::vector<mk_hitlist *> &lists, uint32_t nq, uint32_t nresults, uint32_t q0,
                                  std::vector<uint64_t> &offsets, std::vector<mk_hit> &hits)
{
    std::vector<mk_hit> full;
    for (uint32_t q = 0; q < nq; ++q) {
        full.clear();
        for (mk_hitlist *l : lists) {
            const uint64_t *off = mk_hitlist_offsets(l);
            const mk_hit *h = mk_hitlist_hits(l);
            full.insert(full.end(), h + off[q], h + off[q + 1]);
        }
        // (a heap never holds more than the candidates there are: MK_ALL_RESULTS is their number)
        const uint32_t n = (uint32_t)std::min<uint64_t>(nresults, full.size());
        const size_t at = hits.size();
        hits.resize(at + n);
        hits.resize(at + mk_filter_candidates(full.data(), (uint32_t)full.size(), n, hits.data() + at));
        offsets[q0 + q + 1] = hits.size();
    }
}

// filter_results over complete score rows of every shard (Miekki.cpp:376-397 as written): the
// fallback for overflowed rows, NaN intersections and top-N sizes beyond the device selection.  64 queries at a time.
// Sequences: mk_query_scores.  Indexed genomes: mk_qset_scores over `sets` when they are given (sets of exactly idx[]),
// else over sets made for each step.
int DeviceGroup::replay(const Queries &qy, const std::vector<uint32_t> &idx, std::vector<mk_qset *> *sets, uint32_t nresults,
                        uint32_t min_score, double min_inter, mk_hit *hits, uint32_t *nhits, std::string &err)
{
    const size_t D = ctx_.size();
    const uint32_t step = 64;
    replayed_queries_ += idx.size();
    for (size_t i0 = 0; i0 < idx.size(); i0 += step) {
        const uint32_t n = (uint32_t)std::min<size_t>(step, idx.size() - i0);
        std::vector<const char *> s;
        std::vector<uint64_t> l;
        std::vector<mk_qset *> own;
        if (qy.ids && !sets && make_sets(qy, idx.data() + i0, n, own, err)) return -1;
        for (uint32_t i = 0; !qy.ids && i < n; ++i) { s.push_back(qy.seqs[idx[i0 + i]]); l.push_back(qy.lens[idx[i0 + i]]); }
        const uint32_t first = qy.ids && sets ? (uint32_t)i0 : 0;    // the step's queries in the sets
        std::vector<std::vector<uint32_t>> sc(D);
        int r = MK_OK;
        for (size_t d = 0; d < D && r == MK_OK; ++d) {
            const uint32_t Gd = base_[d + 1] - base_[d];
            sc[d].assign((size_t)n * Gd + 1, 0);
            if (!Gd) continue;
            void *d_sc = nullptr;
            if (!qy.ids) r = mk_query_scores(ctx_[d], s.data(), l.data(), n, sc[d].data());
            else r = mk_dev_alloc(ctx_[d], (uint64_t)n * Gd * 4, &d_sc);
            if (r == MK_OK && qy.ids) r = mk_qset_scores(ctx_[d], (sets ? *sets : own)[d], first, first + n, (uint32_t *)d_sc);
            if (r == MK_OK && qy.ids) r = mk_sync(ctx_[d]);
            if (r == MK_OK && qy.ids) r = mk_dev_download(ctx_[d], sc[d].data(), d_sc, (uint64_t)n * Gd * 4);
            if (r != MK_OK) err = mk_last_error();
            mk_dev_free(ctx_[d], d_sc);
        }
        free_sets(own);
        if (r != MK_OK) return -1;
        filter_score_rows(sc, n, idx.data() + i0, nresults, min_score, min_inter, hits, nhits);
    }
    return 0;
}

// ---- indexed genomes as queries (mk_qset_from_index / mk_qset_from_columns) ------------------------------------

void DeviceGroup::free_sets(std::vector<mk_qset *> &sets)
{
    for (size_t d = 0; d < sets.size(); ++d)
        if (sets[d]) mk_qset_free(ctx_[d], sets[d]);
    sets.clear();
}

int DeviceGroup::indexed_sets(const uint32_t *ids, uint32_t n, std::vector<mk_qset *> &sets, std::string &err)
{
    const size_t D = ctx_.size(), o = owner(ids[0]);
    sets.assign(D, nullptr);
    auto fail = [&] { err = mk_last_error(); free_sets(sets); return -1; };
    if (mk_qset_from_index(ctx_[o], ids, n, &sets[o]) != MK_OK) return fail();
    if (D == 1) return 0;
    mk_params p;
    if (mk_get_params(ctx_[o], &p) != MK_OK) return fail();
    const uint64_t bytes = ((uint64_t)1 << p.h) * n * (p.fp_bits / 8);
    void *d_block = nullptr;
    if (mk_dev_alloc(ctx_[o], bytes, &d_block) != MK_OK) return fail();
    int rc = mk_index_export_genomes_device(ctx_[o], ids, n, (uint8_t *)d_block);
    for (size_t d = 0; d < D && rc == MK_OK; ++d) {
        if (d == o) continue;
        void *d_copy = nullptr;
        rc = mk_dev_alloc(ctx_[d], bytes, &d_copy);
        if (rc == MK_OK) rc = mk_dev_copy(ctx_[d], d_copy, ctx_[o], d_block, bytes);
        if (rc == MK_OK) rc = mk_qset_from_columns(ctx_[d], (const uint8_t *)d_copy, n, &sets[d]);   // (keeps its own copy)
        if (rc != MK_OK) err = mk_last_error();
        mk_dev_free(ctx_[d], d_copy);
        if (rc == MK_OK) gather_bytes_ += bytes;
    }
    if (rc != MK_OK && err.empty()) err = mk_last_error();
    mk_dev_free(ctx_[o], d_block);
    if (rc != MK_OK) { free_sets(sets); return -1; }
    return 0;
}

// runs of ids that one shard owns, 64 at most (the gather's unit): f(first position, count)
template <typename F>
static int for_owned_runs(const DeviceGroup &g, const uint32_t *ids, uint32_t n, F f)
{
    for (uint32_t i = 0; i < n;) {
        uint32_t m = 1;
        while (i + m < n && m < 64 && g.owner(ids[i + m]) == g.owner(ids[i])) ++m;
        if (f(i, m)) return -1;
        i += m;
    }
    return 0;
}

int DeviceGroup::query_indexed(const uint32_t *ids, uint32_t n, uint32_t nresults, uint32_t min_score, double min_inter, mk_hit *hits,
                               uint32_t *nhits, std::string &err)
{
    if (comm_) { err = "indexed genomes are not queried across processes"; return -1; }
    for (uint32_t i = 0; i < n; ++i)
        if (ids[i] >= total()) { err = "genome id " + std::to_string(ids[i]) + " is not in this index"; return -1; }
    if (nresults > 64) {                                              // (beyond the device selection: the list is the same answer)
        std::vector<uint64_t> off;
        std::vector<mk_hit> h;
        if (query_indexed_list(ids, n, nresults, min_score, min_inter, off, h, err)) return -1;
        for (uint32_t i = 0; i < n; ++i) {
            nhits[i] = (uint32_t)(off[i + 1] - off[i]);
            std::copy(h.begin() + off[i], h.begin() + off[i + 1], hits + (size_t)i * nresults);
        }
        return 0;
    }
    const uint32_t cap = row_cap(nresults);
    return for_owned_runs(*this, ids, n, [&](uint32_t i0, uint32_t m) {
        std::vector<uint32_t> pos(m);
        std::iota(pos.begin(), pos.end(), i0);
        return sharded_pass(Queries{nullptr, nullptr, ids}, pos, nresults, min_score, min_inter, hits, nhits, cap, err);
    });
}

int DeviceGroup::query_indexed_list(const uint32_t *ids, uint32_t n, uint32_t nresults, uint32_t min_score, double min_inter,
                                    std::vector<uint64_t> &offsets, std::vector<mk_hit> &hits, std::string &err)
{
    offsets.assign((size_t)n + 1, 0);
    hits.clear();
    if (comm_) { err = "indexed genomes are not queried across processes"; return -1; }
    for (uint32_t i = 0; i < n; ++i)
        if (ids[i] >= total()) { err = "genome id " + std::to_string(ids[i]) + " is not in this index"; return -1; }
    const uint32_t per_shard = ctx_.size() == 1 ? nresults : MK_LIST_CANDIDATES;
    return for_owned_runs(*this, ids, n, [&](uint32_t i0, uint32_t m) {
        std::vector<mk_qset *> sets;
        if (indexed_sets(ids + i0, m, sets, err)) return -1;
        const int ret = merged_lists(m, nresults, i0, [&](size_t d, mk_hitlist **out) {
            return mk_qset_run_list(ctx_[d], sets[d], per_shard, min_score, min_inter, out);
        }, offsets, hits, err);
        free_sets(sets);
        return ret;
    });
}

int DeviceGroup::representatives(uint32_t min_score, double min_inter, std::vector<uint32_t> &rep, std::string &err)
{
    if (comm_) { err = "representatives are not computed across processes"; return -1; }
    if (ctx_.size() > 1) { err = "representatives are not computed across several GPUs"; return -1; }
    rep.assign(total(), 0);
    if (rep.empty()) return 0;
    if (mk_index_representatives(ctx_[0], min_score, min_inter, rep.data()) != MK_OK) { err = mk_last_error(); return -1; }
    return 0;
}

int DeviceGroup::families(uint32_t min_score, double min_inter, std::vector<uint32_t> &labels, std::string &err)
{
    if (comm_) { err = "families are not computed across processes"; return -1; }
    const uint32_t G = total();
    labels.assign(G, 0);
    if (!G) return 0;
    const size_t D = ctx_.size();
    if (D == 1) {
        if (mk_index_families(ctx_[0], min_score, min_inter, labels.data()) != MK_OK) { err = mk_last_error(); return -1; }
        return 0;
    }
    std::vector<void *> forest(D, nullptr);
    void *d_other = nullptr;
    auto release = [&] {
        for (size_t d = 0; d < D; ++d) mk_dev_free(ctx_[d], forest[d]);
        mk_dev_free(ctx_[0], d_other);
    };
    auto fail = [&] { if (err.empty()) err = mk_last_error(); release(); return -1; };
    const uint64_t bytes = (uint64_t)G * 4;
    for (size_t d = 0; d < D; ++d)
        if (mk_dev_alloc(ctx_[d], bytes, &forest[d]) != MK_OK || mk_link_reset(ctx_[d], (uint32_t *)forest[d], G) != MK_OK) return fail();
    std::vector<uint32_t> ids(G);
    std::iota(ids.begin(), ids.end(), 0u);
    const int rc = for_owned_runs(*this, ids.data(), G, [&](uint32_t i0, uint32_t m) {
        std::vector<mk_qset *> sets;
        if (indexed_sets(ids.data() + i0, m, sets, err)) return -1;
        const int r = on_shards(D, err, nullptr, [&](size_t d) {
            const int rd = mk_qset_run_link(ctx_[d], sets[d], ids.data() + i0, min_score, min_inter, (uint32_t *)forest[d], G);
            return rd == MK_OK ? mk_sync(ctx_[d]) : rd;
        });
        free_sets(sets);
        return r;
    });
    if (rc) return fail();
    if (mk_dev_alloc(ctx_[0], bytes, &d_other) != MK_OK) return fail();
    for (size_t d = 1; d < D; ++d) {
        if (mk_dev_copy(ctx_[0], d_other, ctx_[d], forest[d], bytes) != MK_OK || mk_link_merge(ctx_[0], (uint32_t *)forest[0], (const uint32_t *)d_other, G) != MK_OK ||
            mk_sync(ctx_[0]) != MK_OK) return fail();                 // (d_other is the next shard's)
        gather_bytes_ += bytes;
    }
    if (mk_link_labels(ctx_[0], (const uint32_t *)forest[0], G, labels.data()) != MK_OK) return fail();
    release();
    return 0;
}

// ---- the multi-process form: one shard here, the others behind the communicator -------------------------------

int DeviceGroup::all_gather_bytes(const void *mine, uint64_t bytes, std::vector<uint8_t> &all, std::string &err)
{
    const int W = world();
    all.assign(bytes * W, 0);
    if (!bytes) return 0;
    void *d = nullptr;
    if (mk_dev_alloc(ctx_[0], bytes * (W + 1), &d) != MK_OK) { err = mk_last_error(); return -1; }
    int rc = 0;
    if (mk_dev_upload(ctx_[0], (uint8_t *)d + bytes * W, mine, bytes) != MK_OK ||
        mk_comm_allgather(comm_, (uint8_t *)d + bytes * W, bytes, d) != MK_OK ||
        mk_dev_download(ctx_[0], all.data(), d, bytes * W) != MK_OK) { err = mk_last_error(); rc = -1; }
    mk_dev_free(ctx_[0], d);
    return rc;
}

int DeviceGroup::all_gather_text(const std::string &mine, std::vector<std::string> &all, std::string &err)
{
    const int W = world();
    all.assign(W, std::string());
    if (!comm_) { all[0] = mine; return 0; }
    const uint64_t len = mine.size();
    std::vector<uint8_t> lens;
    if (all_gather_bytes(&len, 8, lens, err)) return -1;
    uint64_t mx = 0;
    std::vector<uint64_t> n(W);
    for (int r = 0; r < W; ++r) { memcpy(&n[r], lens.data() + 8 * r, 8); mx = std::max(mx, n[r]); }
    if (!mx) return 0;
    std::vector<uint8_t> padded(mx, 0), got;
    memcpy(padded.data(), mine.data(), mine.size());
    if (all_gather_bytes(padded.data(), mx, got, err)) return -1;
    for (int r = 0; r < W; ++r) all[r].assign((const char *)got.data() + mx * r, n[r]);
    return 0;
}

// One pass: every rank scans the batch against its shard and the entrant rows travel to rank 0 while the scan goes on
// (mk_qset_run_compact_gather: ncclGather, or grouped send / recv blocks); rank 0 merges on its GPU and tells everybody
// which rows overflowed; those run once more with wide rows, and what overflows even then is answered from dense rows.
int DeviceGroup::query_ranked(const std::vector<uint32_t> &idx, const char *const *seqs, const uint64_t *lens, uint32_t nresults,
                              uint32_t min_score, double min_inter, mk_hit *hits, uint32_t *nhits, uint32_t cap, std::string &err)
{
    mk_ctx *c = ctx_[0];
    const int W = world();
    const uint32_t n = (uint32_t)idx.size();
    std::vector<const char *> s(n);
    std::vector<uint64_t> l(n);
    for (uint32_t i = 0; i < n; ++i) { s[i] = seqs[idx[i]]; l[i] = lens[idx[i]]; }
    const uint64_t words = (uint64_t)n * (cap + 1);
    void *d_rows = nullptr, *d_recv = nullptr, *d_hits = nullptr, *d_nh = nullptr, *d_over = nullptr;
    mk_qset *qs = nullptr;
    std::vector<uint32_t> over_msg(n + 1, 0);                         // [count, positions in idx ...]: rank 0 -> everybody
    auto cleanup = [&] {
        if (qs) mk_qset_free(c, qs);
        mk_dev_free(c, d_rows); mk_dev_free(c, d_recv); mk_dev_free(c, d_hits); mk_dev_free(c, d_nh); mk_dev_free(c, d_over);
    };
    auto fail = [&] { err = mk_last_error(); cleanup(); return -1; };
    // what only this rank does -- buffers, the upload and sketch of the queries -- may fail on this rank alone: every rank
    // says how it fared BEFORE the gather, and all leave together if one could not (nobody waits in a collective the failed
    // rank never enters)
    bool ready = mk_dev_alloc(c, words * 8, &d_rows) == MK_OK && mk_dev_alloc(c, (uint64_t)(n + 1) * 4, &d_over) == MK_OK;
    if (ready && root())
        ready = mk_dev_alloc(c, words * 8 * W, &d_recv) == MK_OK && mk_dev_alloc(c, (uint64_t)n * 4, &d_nh) == MK_OK &&
                mk_dev_alloc(c, (uint64_t)n * std::max(nresults, 1u) * sizeof(mk_hit), &d_hits) == MK_OK;
    ready = ready && mk_qset_upload(c, s.data(), l.data(), n, &qs) == MK_OK;
    {
        const std::string mine = ready ? std::string() : std::string("rank ") + std::to_string(rank()) + ": " + mk_last_error();
        std::vector<std::string> all;
        if (all_gather_text(mine, all, err)) { cleanup(); return -1; }
        for (const std::string &e : all)
            if (!e.empty()) { err = e; cleanup(); return -1; }
    }
    if (mk_qset_run_compact_gather(c, comm_, qs, nresults, min_score, min_inter, cap, (uint64_t *)d_rows, (uint64_t *)d_recv, 0) != MK_OK) return fail();
    constexpr uint32_t kRootFailed = 0xFFFFFFFFu;                     // (rank 0's own failure travels in the message everybody waits for)
    if (root()) {
        gather_bytes_ += (uint64_t)(W - 1) * words * 8;
        std::vector<uint32_t> nh(n);
        std::vector<mk_hit> hh((size_t)n * std::max(nresults, 1u));
        const bool merged = mk_merge_compact(c, (const uint64_t *)d_recv, (uint32_t)W, n, cap, nresults, (mk_hit *)d_hits, (uint32_t *)d_nh) == MK_OK &&
                            mk_dev_download(c, nh.data(), d_nh, (uint64_t)n * 4) == MK_OK &&
                            (!nresults || mk_dev_download(c, hh.data(), d_hits, (uint64_t)n * nresults * sizeof(mk_hit)) == MK_OK);
        if (!merged) { err = mk_last_error(); over_msg[0] = kRootFailed; }
        for (uint32_t i = 0; merged && i < n; ++i) {
            if (nh[i] == MK_MERGE_OVERFLOW) { over_msg[++over_msg[0]] = i; continue; }
            nhits[idx[i]] = nh[i];
            std::copy(hh.begin() + (size_t)i * nresults, hh.begin() + (size_t)i * nresults + nh[i], hits + (size_t)idx[i] * nresults);
        }
        if (mk_dev_upload(c, d_over, over_msg.data(), (uint64_t)(n + 1) * 4) != MK_OK) return fail();
    }
    if (mk_comm_broadcast(comm_, d_over, (uint64_t)(n + 1) * 4, 0) != MK_OK ||
        mk_dev_download(c, over_msg.data(), d_over, (uint64_t)(n + 1) * 4) != MK_OK) return fail();
    if (over_msg[0] == kRootFailed) { if (err.empty()) err = "rank 0 could not merge the rows"; cleanup(); return -1; }
    cleanup();
    qs = nullptr; d_rows = d_recv = d_hits = d_nh = d_over = nullptr;
    if (!over_msg[0]) return 0;
    std::vector<uint32_t> over;
    for (uint32_t i = 1; i <= over_msg[0]; ++i) over.push_back(idx[over_msg[i]]);
    static const bool wide = [] { const char *e = getenv("MIEKKI_SHARD_WIDE_ROWS"); return !e || atoi(e) != 0; }();
    if (wide && cap < kCapWide) {
        rerun_queries_ += over.size();
        for (size_t i0 = 0; i0 < over.size(); i0 += 4096) {
            const std::vector<uint32_t> piece(over.begin() + i0, over.begin() + std::min(over.size(), i0 + 4096));
            if (query_ranked(piece, seqs, lens, nresults, min_score, min_inter, hits, nhits, kCapWide, err)) return -1;
        }
        return 0;
    }
    return replay_ranked(over, seqs, lens, nresults, min_score, min_inter, hits, nhits, err);
}

// filter_results over complete score rows (Miekki.cpp:376-397 as written): every rank's dense rows of the queries,
// padded to the largest shard, gathered on rank 0 (ncclGather), which walks them in rank = genome order
int DeviceGroup::replay_ranked(const std::vector<uint32_t> &idx, const char *const *seqs, const uint64_t *lens, uint32_t nresults,
                               uint32_t min_score, double min_inter, mk_hit *hits, uint32_t *nhits, std::string &err)
{
    mk_ctx *c = ctx_[0];
    const int W = world();
    const uint32_t step = 64, Gmine = mk_index_size(c);
    replayed_queries_ += idx.size();
    const uint32_t mine = Gmine;
    std::vector<uint8_t> counts;
    if (all_gather_bytes(&mine, 4, counts, err)) return -1;
    std::vector<uint32_t> Gr(W), first(W + 1, 0);
    for (int r = 0; r < W; ++r) { memcpy(&Gr[r], counts.data() + 4 * r, 4); first[r + 1] = first[r] + Gr[r]; }
    const uint64_t pitch = std::max<uint32_t>(largest_shard_, 1);
    void *d_send = nullptr, *d_recv = nullptr;
    if (mk_dev_alloc(c, (uint64_t)step * pitch * 4, &d_send) != MK_OK ||
        (root() && mk_dev_alloc(c, (uint64_t)step * pitch * 4 * W, &d_recv) != MK_OK)) { err = mk_last_error(); mk_dev_free(c, d_send); return -1; }
    int rc = 0;
    std::vector<uint32_t> sc((size_t)step * pitch), all;
    if (root()) all.resize((size_t)step * pitch * W);
    for (size_t i0 = 0; i0 < idx.size() && !rc; i0 += step) {
        const uint32_t n = (uint32_t)std::min<size_t>(step, idx.size() - i0);
        std::vector<const char *> s(n);
        std::vector<uint64_t> l(n);
        for (uint32_t i = 0; i < n; ++i) { s[i] = seqs[idx[i0 + i]]; l[i] = lens[idx[i0 + i]]; }
        std::fill(sc.begin(), sc.end(), 0u);
        if (Gmine) {
            std::vector<uint32_t> dense((size_t)n * Gmine);
            if (mk_query_scores(c, s.data(), l.data(), n, dense.data()) != MK_OK) { err = mk_last_error(); rc = -1; break; }
            for (uint32_t i = 0; i < n; ++i) memcpy(sc.data() + (size_t)i * pitch, dense.data() + (size_t)i * Gmine, (size_t)Gmine * 4);
        }
        const uint64_t bytes = (uint64_t)step * pitch * 4;
        if (mk_dev_upload(c, d_send, sc.data(), bytes) != MK_OK || mk_comm_gather(comm_, d_send, bytes, d_recv, 0) != MK_OK ||
            (root() ? mk_dev_download(c, all.data(), d_recv, bytes * W) : mk_sync(c)) != MK_OK) { err = mk_last_error(); rc = -1; break; }
        if (!root()) continue;
        std::vector<mk_hit> full;
        for (uint32_t i = 0; i < n; ++i) {
            full.clear();
            for (int r = 0; r < W; ++r) {
                const uint32_t *row = all.data() + ((size_t)r * step + i) * pitch;
                for (uint32_t g = 0; g < Gr[r]; ++g) {
                    if (row[g] < min_score) continue;
                    const uint32_t id = first[r] + g;
                    const double jac = (double)row[g] / ss_all_[id];
                    const double inter = jac * gs_all_[id];
                    if (inter < min_inter) continue;
                    full.push_back(mk_hit{id, row[g], jac, inter});
                }
            }
            const uint32_t q = idx[i0 + i];
            nhits[q] = mk_filter_candidates(full.data(), (uint32_t)full.size(), nresults, hits + (size_t)q * nresults);
        }
    }
    mk_dev_free(c, d_send);
    mk_dev_free(c, d_recv);
    return rc;
}

}  // namespace mkhost
