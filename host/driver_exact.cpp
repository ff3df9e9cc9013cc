// The exact mode of the `miekki` binary, -e: the hits of the index verified against the genomes' files
// (Miekki.cpp:723-859).
#include "driver.hpp"

#include <cstring>
#include <future>
#include <unordered_map>

using namespace std;

namespace mkhost {

// ---- exact mode: the hits of a fixed-width query, verified against the genomes' files

namespace {

bool nucleotide_start(const string &s)           // Miekki.cpp:736, 771
{
    return !s.empty() && (s[0] == 'A' || s[0] == 'C' || s[0] == 'G' || s[0] == 'T' || s[0] == 'N');
}

// strict 2-line records (Miekki.cpp:458-464)
void read_records(const string &path, vector<string> &heads, vector<string> &seqs)
{
    string text;
    mkhost::read_text(path, text);
    vector<string> lines = split_lines(text);
    for (size_t i = 0; i < lines.size(); i += 2) {
        heads.push_back(std::move(lines[i]));
        seqs.push_back(i + 1 < lines.size() ? std::move(lines[i + 1]) : string());
    }
}

}  // namespace

// a genome file as ground_truth_batch sees it: contigs split at '>' lines (Miekki.cpp:805-812),
// walked line by line over the raw text.  Callable from a helper thread.
Driver::GenomeContigs Driver::parse_contigs(const string &file) const
{
    GenomeContigs gc;
    gc.exists = mkhost::file_exists(file);
    if (!gc.exists) return gc;
    vector<char> text, scratch;
    mkhost::read_file(file, text, scratch);
    string ref;
    ref.reserve(text.size());
    const char *pos = text.data(), *const end = text.data() + text.size();
    while (pos <= end) {                                                     // getline semantics
        const char *e = pos < end ? (const char *)memchr(pos, '\n', (size_t)(end - pos)) : nullptr;
        if (!e) e = end;
        if (e != pos && *pos == '>') {
            if (ref.size() >= k) { gc.contigs.push_back(std::move(ref)); ref = string(); }   // short contigs leak (806-812)
        } else {
            ref.append(pos, (size_t)(e - pos));
        }
        pos = e + 1;
    }
    if (ref.size() >= k) gc.contigs.push_back(std::move(ref));
    return gc;
}

// ground_truth_batch (Miekki.cpp:792-859) for all pending queries of one genome file.  The
// reference rebuilds the file's k-mer set at every call (~7 s); here the set stays resident on
// the GPU that verified the file last, so a file whose queries are flushed in several batches
// (the flush-at-100 rule) is read, split and hashed once.
mk_ctx *Driver::exact_ctx(const vector<ExactPending> &v, size_t &shard)
{
    // K7 runs on the GPU that owns the genome (any would do: the sets come from the file itself)
    shard = v.empty() || group.ranked() ? 0 : group.owner(v[0].genome);
    if (resident.size() != group.shards()) resident.assign(group.shards(), string());
    return group.ctx(shard);
}
bool Driver::is_resident(const string &file, const vector<ExactPending> &v)
{
    size_t shard;
    exact_ctx(v, shard);
    return !file.empty() && resident[shard] == file;
}

void Driver::ground_truth(const string &file, const vector<ExactPending> &v)
{
    if (is_resident(file, v)) ground_truth(file, v, GenomeContigs{});
    else ground_truth(file, v, parse_contigs(file));
}

void Driver::ground_truth(const string &file, const vector<ExactPending> &v, const GenomeContigs &gc)
{
    size_t shard;
    mk_ctx *ctx = exact_ctx(v, shard);
    if (resident[shard] != file) {
        if (!gc.exists) { cout << "File problem: " << file << endl; return; }
        vector<const char *> cp;
        vector<uint64_t> cl;
        for (auto &c : gc.contigs) { cp.push_back(c.data()); cl.push_back(c.size()); }
        resident[shard].clear();
        if (mk_exact_load_genome(ctx, cp.data(), cl.data(), (uint32_t)gc.contigs.size()) != MK_OK) die("exact mode failed");
        resident[shard] = file;
    }
    vector<const char *> qp;
    vector<uint64_t> ql;
    for (auto &q : v) { qp.push_back(q.seq.data()); ql.push_back(q.seq.size()); }
    vector<uint64_t> inter(v.size()), uni(v.size());
    if (mk_exact_query(ctx, qp.data(), ql.data(), (uint32_t)v.size(), inter.data(), uni.data()) != MK_OK)
        die("exact mode failed");
    for (size_t i = 0; i < v.size(); ++i) {
        if (!inter[i]) continue;                                             // 843
        const double real_jax = (double)inter[i] / (double)uni[i];
        out << real_jax << "\t" << v[i].jaccard << "\t" << (double)inter[i] << "\t" << v[i].intersection
            << "\t" << v[i].head << "\t" << file << "\n";                    // 853
    }
}

bool Driver::need_names()
{
    if (file_names.size() == group.total()) return true;
    cout << "exact mode needs the genome files of the index: build it with -l in the same run "
            "(file names are not stored in an index file)" << endl;
    return false;
}

void Driver::exact_collect(const vector<string> &heads, const vector<const string *> &seqs, uint32_t nres,
                   uint32_t min_score)
{
    vector<const char *> p;
    vector<uint64_t> l;
    for (auto s : seqs) { p.push_back(s->data()); l.push_back(s->size()); }
    Answers a;
    query_fixed(p, l, nres, min_score, (double)threshold, a);
    if (!group.root()) return;                                   // (one process per GPU: rank 0 verifies and writes)
    // Same container, same insertion sequence and the same flush-at-100 rule as the
    // reference (Miekki.cpp:728-754, 779-785): with the same libstdc++ the lines of the
    // output file then come out in the reference's order, not just as the same set.
    unordered_map<string, vector<ExactPending>> batch;
    for (size_t q = 0; q < seqs.size(); ++q)
        for (uint32_t i = 0; i < a.nhits[q]; ++i) {
            const mk_hit &h = a.hits[a.begin[q] + i];
            const string &file_name = file_names[h.genome];
            vector<ExactPending> &v = batch[file_name];
            v.push_back(ExactPending{*seqs[q], heads[q], h.jaccard, h.intersection, h.genome});
            if (v.size() >= 100) { ground_truth(file_name, v); v.clear(); }
        }
    // the genome file of the NEXT entry is read and split while the device works on this one
    vector<const std::pair<const string, vector<ExactPending>> *> todo;
    for (auto itr = batch.begin(); itr != batch.end(); ++itr)
        if (!itr->second.empty()) todo.push_back(&*itr);
    std::future<GenomeContigs> ahead;
    // (a file whose set is still resident from a flush above is not read again)
    auto parse_unless_resident = [this](const string &f, bool res) { return res ? GenomeContigs{} : parse_contigs(f); };
    if (!todo.empty())
        ahead = std::async(std::launch::async, parse_unless_resident, todo[0]->first, is_resident(todo[0]->first, todo[0]->second));
    for (size_t i = 0; i < todo.size(); ++i) {
        GenomeContigs gc = ahead.get();
        if (i + 1 < todo.size())
            ahead = std::async(std::launch::async, parse_unless_resident, todo[i + 1]->first, false);
        ground_truth(todo[i]->first, todo[i]->second, gc);
    }
    out << flush;
}

// ---- Miekki.cpp:723-759
void Driver::query_file_exact(const string &path)
{
    if (!mkhost::file_exists(path)) { cout << "File problem" << endl; return; }
    if (!need_names()) return;
    vector<string> heads, seqs, kh;
    read_records(path, heads, seqs);
    vector<const string *> kept;
    for (size_t i = 0; i < seqs.size(); ++i)
        if (seqs[i].size() >= k && nucleotide_start(seqs[i])) { kept.push_back(&seqs[i]); kh.push_back(heads[i]); }
    exact_collect(kh, kept, 5, 10);
}

// ---- Miekki.cpp:616-645, 763-788
void Driver::query_file_of_file_exact(const string &list)
{
    if (!mkhost::file_exists(list)) { cout << "Missed file of file: " << list << endl; return; }
    if (!need_names()) return;
    vector<string> heads, refs;
    for (const string &fn : read_list(list)) {
        if (!mkhost::file_exists(fn)) {
            cout << "File problem" << endl;
        } else {
            string ftext;
            mkhost::read_text(fn, ftext);
            vector<string> lines = split_lines(ftext);
            string ref;
            for (size_t i = 1; i < lines.size(); ++i)
                if (lines[i].size() >= k && nucleotide_start(lines[i])) ref += lines[i];   // 771-775
            heads.push_back(lines.empty() ? string() : lines[0]);
            refs.push_back(std::move(ref));
        }
        cout << "-" << flush_stream();
    }
    vector<const string *> ptrs;
    for (auto &r : refs) ptrs.push_back(&r);
    exact_collect(heads, ptrs, 5, 5);
}

}  // namespace mkhost
