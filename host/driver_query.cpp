// The query modes of the `miekki` binary: -a (query_file), -A (query_file_of_file), and the flags that are not in the
// reference and read or answer the same way:
//   * -X (no argument; not in the reference): every genome of the index against the index, answered from the genomes'
//     stored columns -- what -A over the indexed files themselves prints, without the files (query_index below).
//   * -F <file> (not in the reference): the families the indexed genomes fall into -- connected components of "one is
//     among the other's hits above -X's thresholds" -- computed on the device (write_families below).
//   * -R <file>, -r <file> (not in the reference): greedy representatives over the same links, earlier ids first -- the
//     genomes to keep (a -K list), and the clusters around them (write_representatives below).  One GPU.
//   * -J <levels> -H <file> -O <file> (not in the reference): the nested families at several thresholds from one pass, as
//     a taxonomy for -T and the order for -K that makes its nodes runs of ids (write_hierarchy below).  One GPU.
//   * -2 <file> with -a (not in the reference; Kraken's --paired): the mates of -a's records, the i-th of one file with the
//     i-th of the other -- a pair is ONE query of the approximate mode and of every flag below over -a's reads: its k-mers
//     are those of each mate alone, mate 1 wins a tie, the Bloom gate is asked for the winner (mk_qset_upload_pairs;
//     host/reads.hpp).  Marks, -Y's ordinals and the summaries count pairs; the head printed is mate 1's.  One GPU.
//   * FASTQ (not in the reference): a read file of -a, -2 or -S whose first byte, after inflation, is '@' and whose third line starts with '+' is read as four-line
//     records, run as their sequences and printed under their head lines, '@' included (host/reads.hpp).  -q <int> with such
//     files (Kraken 2's --minimum-base-quality): the qualities go up with the reads, and the device cuts every read at the
//     bases below <int> -- its k-mers are those of each stretch of good bases alone, the read stays one query
//     (mk_qset_upload_reads); stdout gets one `quality:` line.  One GPU, at most 4,096 bases per read or pair.
#include "driver.hpp"

#include <future>

#include "families.hpp"
#include "hierarchy.hpp"

using namespace std;

namespace mkhost {

// One fixed-width call for sequences on the group: `width` slots per query (Miekki.cpp:437, 500; the exact mode's five)
void Driver::query_fixed(const vector<const char *> &p, const vector<uint64_t> &l, uint32_t width, uint32_t min_score, double min_inter, Answers &a)
{
    a.fixed(p.size(), width);
    if (p.empty()) return;
    string err;
    if (group.query(p.data(), l.data(), (uint32_t)p.size(), width, min_score, min_inter, a.hits.data(), a.nhits.data(), err) != 0) {
        cout << "query failed: " << err << endl;
        exit(1);
    }
}

// The approximate mode's call, filter_results(query_sequences(batch), nres, 10, 0.5 * threshold) (Miekki.cpp:437, 500), at its
// three entry points -- sequences on the group, a batch as a set on the first context, indexed ids: the reference's ten
// through the fixed-width path, any other -n as a list.
void Driver::answer(const vector<const char *> &p, const vector<uint64_t> &l, Answers &a)
{
    if (nres == 10) { query_fixed(p, l, 10, 10, 0.5 * threshold, a); return; }
    vector<uint64_t> off(p.size() + 1, 0);
    string err;
    a.hits.clear();
    if (!p.empty() && group.query_list(p.data(), l.data(), (uint32_t)p.size(), nres, 10, 0.5 * threshold, off, a.hits, err) != 0) {
        cout << "query failed: " << err << endl;
        exit(1);
    }
    a.from_offsets(off.data(), p.size());
}

// a batch of for_read_batches as a set on a context: reads, pairs (-2: mk_qset_upload_pairs), and with -q either with their
// base qualities (mk_qset_upload_reads)
void Driver::upload_batch(mk_ctx *ctx, const ReadBatch &b, const char *fail, mk_qset **qs)
{
    const uint32_t n = (uint32_t)b.q.size();
    if (min_qual >= 0) {
        const bool paired = !mates.empty();
        must(mk_qset_upload_reads(ctx, b.q.data(), b.ql.data(), b.qual_q.data(), paired ? b.mate_q.data() : nullptr, paired ? b.mate_ql.data() : nullptr,
                                  paired ? b.mate_qual_q.data() : nullptr, n, (uint32_t)min_qual, qs), "-q: the upload failed");
    } else if (mates.empty()) must(mk_qset_upload(ctx, b.q.data(), b.ql.data(), n, qs), fail);
    else must(mk_qset_upload_pairs(ctx, b.q.data(), b.ql.data(), b.mate_q.data(), b.mate_ql.data(), n, qs), "-2: the upload failed");
}

// ... for the pairs of -2, each ONE query, and for -q's reads or pairs with qualities, on the one context -2 and -q run with
// (a set is answered as a list whatever -n is)
void Driver::answer_batch(const ReadBatch &b, Answers &a)
{
    if (mates.empty() && min_qual < 0) { answer(b.q, b.ql, a); return; }
    const size_t n = b.q.size();
    a.hits.clear();
    if (!n) { a.from_offsets(nullptr, 0); return; }
    mk_qset *qs = nullptr;
    mk_hitlist *list = nullptr;
    upload_batch(ctx0(), b, "-q: the upload failed", &qs);
    must(mk_qset_run_list(ctx0(), qs, nres, 10, 0.5 * threshold, &list), min_qual >= 0 ? "-q: query failed" : "-2: query failed");
    const uint64_t *off = mk_hitlist_offsets(list);
    const mk_hit *h = mk_hitlist_hits(list);
    a.hits.assign(h, h + off[n]);
    a.from_offsets(off, n);
    mk_hitlist_free(list);
    mk_qset_free(ctx0(), qs);
}

void Driver::answer_indexed(const vector<uint32_t> &ids, Answers &a)
{
    const uint32_t m = (uint32_t)ids.size();
    string err;
    int rc;
    if (nres == 10) {
        a.fixed(m, 10);
        rc = group.query_indexed(ids.data(), m, 10, 10, 0.5 * threshold, a.hits.data(), a.nhits.data(), err);   // 500
    } else {
        vector<uint64_t> off;
        rc = group.query_indexed_list(ids.data(), m, nres, 10, 0.5 * threshold, off, a.hits, err);
        if (rc == 0) a.from_offsets(off.data(), m);
    }
    if (rc != 0) { cout << "query failed: " << err << endl; exit(1); }
}

// The one reader loop over a query file: fn(batch) for its records in super-batches; the next one is read and split while
// fn -- the device -- works on this one.  After a batch, one mark per reference batch (345).  Returns the number of records.
// With -2 the records are PAIRS, with -q they come with their qualities, which are counted here (ReadBatch).
size_t Driver::for_read_batches(const string &path, const std::function<void(ReadBatch &)> &fn)
{
    RecordStream in(path);
    std::unique_ptr<PairStream> pairs(mates.empty() ? nullptr : new PairStream(in, path, mates));
    const bool masked = min_qual >= 0;
    if (masked) (pairs ? pairs->max_bases : in.max_bases) = mkhost::kQualityBasesMax;
    const size_t super = kSuperBatch;
    ReadBatch batch, next;
    size_t done = 0;
    auto read = [&](ReadBatch &b) {
        return pairs ? pairs->next(super, k, b.heads, b.seqs, b.mates, masked ? &b.quals : nullptr, masked ? &b.mate_quals : nullptr)
                     : in.next(super, k, b.heads, b.seqs, masked ? &b.quals : nullptr);
    };
    // (a mate file that ends early, a pair beyond the short sketch, a FASTQ record that is none, with -q a read beyond the
    // masked sketch: the run ends there, before any sink's file is written)
    auto refuse = [&] {
        const string &why = pairs ? pairs->error : in.error;
        if (!why.empty()) { cout << why << endl; exit(1); }
    };
    bool more = read(batch);
    refuse();
    while (more) {
        auto ahead = std::async(std::launch::async, [&] { return read(next); });
        batch.point();
        if (masked)
            for (size_t i = 0; i < batch.quals.size(); ++i) {
                if (pairs) quality.pair(batch.quals[i], batch.mate_quals[i], k, (uint32_t)min_qual);
                else quality.read(batch.quals[i], k, (uint32_t)min_qual);
            }
        fn(batch);
        for (size_t i = 0; i < batch.seqs.size(); ++i)
            if (((done + i) % 201) == 0) cout << "-" << flush_stream();
        done += batch.seqs.size();
        more = ahead.get();
        refuse();
        std::swap(batch, next);
    }
    return done;
}

// ---- Miekki.cpp:426-483
void Driver::query_file(const string &path)
{
    if (!mkhost::file_exists(path)) { cout << "File problem" << endl; return; }
    struct WriteJob { vector<string> heads; Answers a; size_t n = 0; };
    std::future<void> writer;
    for_read_batches(path, [&](ReadBatch &b) {
        auto job = std::make_shared<WriteJob>();
        answer_batch(b, job->a);
        // formatting and writing this batch's lines runs beside the next batch's device work
        // (one writer at a time, in order)
        if (writer.valid()) writer.get();
        job->heads.swap(b.heads);
        job->n = b.seqs.size();
        writer = std::async(std::launch::async, [this, job] {
            string text;
            for (size_t i = 0; i < job->n; ++i) {
                text += job->heads[i];
                text += ':';
                text += hit_text(job->a.hits.data() + job->a.begin[i], job->a.nhits[i]);
                text += '\n';
            }
            out << text;
        });
    });
    if (writer.valid()) writer.get();
    out << flush;
    print_quality();
}

// ---- Miekki.cpp:592-612, 487-514
void Driver::query_file_of_file(const string &list)
{
    if (!mkhost::file_exists(list)) { cout << "Missed file of file: " << list << endl; return; }
    const vector<string> files = read_list(list);
    // readers parse into pinned buffers, two batches ahead: the upload of a batch is a DMA
    // straight out of them
    PinnedArena arena(ctx0());
    OrderedFastaReader reader(files, threads, mkhost::HostAllocator{pinned_alloc, pinned_free, &arena}, 2 * 64);
    // whole files are queried 64 at a time: the dense kernel scores sixteen per wave and lets the four waves of a workgroup
    // walk the same rows together (the later sets find them in the Infinity Cache): 80 ms for 64 queries against 100,000 genomes, 44 ms for 32; output stays
    // in list order
    vector<string> names;
    vector<OrderedFastaReader::Item> refs;
    uint64_t bytes = 0;
    auto flush = [&]() {
        if (refs.empty()) return;
        vector<const char *> p;
        vector<uint64_t> l;
        for (auto &r : refs) { p.push_back(r.data); l.push_back(r.len); }
        Answers a;
        answer(p, l, a);
        for (size_t i = 0; i < refs.size(); ++i)
            if (a.nhits[i]) out << names[i] << ":" << hit_text(a.hits.data() + a.begin[i], a.nhits[i]) << "\n";   // 506-511
        out << std::flush;
        for (auto &r : refs) reader.recycle(r);
        names.clear(); refs.clear(); bytes = 0;
    };
    for (size_t i = 0; i < files.size(); ++i) {
        OrderedFastaReader::Item item = reader.take(i);
        if (!item.exists) {
            cout << "File problem" << endl;
            reader.recycle(item);
        } else if (item.failed) {
            cout << "cannot read " << files[i] << endl;
            exit(1);
        } else if (item.len >= k) {
            bytes += item.len;
            names.push_back(files[i]); refs.push_back(item);
            if (refs.size() >= 64 || bytes > (1ull << 30)) flush();
        } else {
            reader.recycle(item);
        }
        cout << "-" << flush_stream();
    }
    flush();
}

// ---- -X: query_whole_file (Miekki.cpp:487-514) for every INDEXED genome, without its file: the genome's stored column
// is the gated sketch query_sequence would compute for its sequence (same minhash_sketch_partition, 281 / 320; the
// Bloom gate passes every active partition of an inserted genome, 295-299 + 135-146).  In id order, 64 genomes at a
// time; a line starts with the genome's file name when this run built the index from a list, else with its id.
void Driver::query_index()
{
    const uint32_t G = group.total();
    const bool named = G && file_names.size() == G;
    vector<uint32_t> ids;
    Answers a;
    for (uint32_t g0 = 0; g0 < G; g0 += 64) {
        const uint32_t m = std::min<uint32_t>(64, G - g0);
        ids.resize(m);
        for (uint32_t i = 0; i < m; ++i) ids[i] = g0 + i;
        answer_indexed(ids, a);
        for (uint32_t i = 0; i < m; ++i) {
            if (a.nhits[i]) {                                                                                   // 506-511
                if (named) out << file_names[g0 + i]; else out << g0 + i;
                out << ":" << hit_text(a.hits.data() + a.begin[i], a.nhits[i]) << "\n";
            }
            cout << "-" << flush_stream();
        }
        out << std::flush;
    }
}

// ---- -F: the families of the indexed genomes at -X's thresholds (mk_index_families; several GPUs: a forest per shard,
// folded on the first), written as a list -K takes: families by ascending label, members ascending, a blank line between
void Driver::write_families(const string &path)
{
    vector<uint32_t> labels;
    string err, text;
    if (group.families(10, 0.5 * threshold, labels, err) != 0) { cout << "-F: families failed: " << err << endl; exit(1); }
    mkhost::FamilyCounts counts;
    if (!mkhost::format_families(labels.data(), labels.size(), text, counts, err)) { cout << "-F: " << err << endl; exit(1); }
    write_text("-F", path, text);
    cout << mkhost::family_summary(counts) << endl;
}

// ---- -R / -r: greedy representatives in id order at -X's thresholds (mk_index_representatives; one context).  -R: the
// representatives ascending, a list -K takes; -r: rep[] has the shape of family labels, so the clusters are written as -F
// writes families -- by ascending representative, which is a cluster's first line
void Driver::write_representatives(const string &reps_path, const string &clusters_path)
{
    vector<uint32_t> rep;
    string err, text;
    if (group.representatives(10, 0.5 * threshold, rep, err) != 0) { cout << "-R / -r: representatives failed: " << err << endl; exit(1); }
    mkhost::FamilyCounts counts;
    if (!mkhost::format_families(rep.data(), rep.size(), text, counts, err)) { cout << "-R / -r: " << err << endl; exit(1); }
    if (!reps_path.empty()) {
        string list;
        for (size_t j = 0; j < rep.size(); ++j)
            if (rep[j] == j) { list += to_string(j); list += '\n'; }
        write_text("-R", reps_path, list);
    }
    if (!clusters_path.empty()) write_text("-r", clusters_path, text);
    cout << "representatives: " << counts.families << " of " << rep.size() << ", largest cluster " << counts.largest << endl;
}

// ---- -J -H -O: the nested families of the indexed genomes at -J's levels from one all-vs-all pass (mk_index_hierarchy; one
// context), laid out by host/hierarchy.hpp: -O the order in which every family of every level is a run of ids, a list -K
// takes; -H the taxonomy over the places in that order, a file -T takes.  The levels are read again here: a level without an
// intersection takes 0.5 * the index's own -s, as -F does, which for -i is the file's and not the command line's.
void Driver::write_hierarchy(const string &levels_arg, const string &taxonomy_path, const string &order_path)
{
    vector<mk_level> levels;
    string err, text;
    if (!mkhost::parse_levels(levels_arg, 0.5 * threshold, levels, err)) { cout << err << endl; exit(1); }
    if (group.shards() > 1 || group.ranked()) { cout << "-J -H -O: the hierarchy is computed on one GPU" << endl; exit(1); }
    const uint32_t L = (uint32_t)levels.size();
    const uint64_t G = group.total();
    vector<uint32_t> labels((size_t)L * G), order;
    if (mk_index_hierarchy(ctx0(), levels.data(), L, labels.data()) != MK_OK) { cout << "-J: hierarchy failed: " << mk_last_error() << endl; exit(1); }
    vector<mkhost::HierarchyNode> nodes;
    if (!mkhost::layout_hierarchy(labels.data(), L, G, order, nodes, err)) { cout << "-J: " << err << endl; exit(1); }
    mkhost::format_hierarchy_order(order, text);
    write_text("-O", order_path, text);
    text.clear();
    mkhost::format_hierarchy_taxonomy(nodes, text);
    write_text("-H", taxonomy_path, text);
    cout << mkhost::hierarchy_summary(labels.data(), L, G, nodes) << endl;
}

}  // namespace mkhost
