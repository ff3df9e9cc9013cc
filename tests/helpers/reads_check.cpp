// Stand-alone check of host/reads.hpp (tests/test_host_reads.py builds it with -fsanitize=address,undefined):
//   reads_check dump <k> <want> <file>          the records next() keeps, `want` at a time: head TAB sequence TAB quality
//   reads_check records <file>                  the records record() hands out, whatever their length
//   reads_check pairs <k> <want> <file1> <file2>  PairStream's: head TAB mate 1 TAB mate 2 TAB quality 1 TAB quality 2
//   reads_check old <k> <want> <file>           the same file through the 2-line reader as it was before FASTQ, and through
//                                               RecordStream: prints `same <records>` or the first difference
//   reads_check quality <k> <q> <file> [<file2>]  the `quality:` line of the file's kept reads (pairs)
//   reads_check isfastq <file>
// A stream's error is printed as `error: <text>` after the records before it.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "reads.hpp"

using std::string;
using std::vector;

// the reader of 2-line records as the command line had it before it learnt FASTQ
class OldRecordStream {
public:
    explicit OldRecordStream(const string &path) : f_(gzopen(path.c_str(), "rb")), buf_(4u << 20)
    {
        if (f_) gzbuffer(f_, 1u << 20);
    }
    ~OldRecordStream() { if (f_) gzclose(f_); }
    bool next(size_t want, uint32_t k, vector<string> &heads, vector<string> &seqs)
    {
        heads.clear(); seqs.clear();
        string head, ref;
        while (seqs.size() < want && !done_) {
            const bool got_head = getline(head);
            const bool got_ref = getline(ref);
            if (!got_head && !got_ref) break;
            if (ref.size() >= k) { heads.push_back(std::move(head)); seqs.push_back(std::move(ref)); }
            head.clear(); ref.clear();
        }
        return !seqs.empty();
    }
private:
    bool getline(string &out)
    {
        out.clear();
        bool any = false;
        for (;;) {
            if (pos_ == len_) {
                if (done_ || !f_) { done_ = true; return any; }
                const int n = gzread(f_, buf_.data(), (unsigned)buf_.size());
                if (n <= 0) { done_ = true; return any; }
                pos_ = 0; len_ = (size_t)n;
            }
            any = true;
            const char *p = buf_.data() + pos_;
            const char *e = (const char *)memchr(p, '\n', len_ - pos_);
            if (e) { out.append(p, (size_t)(e - p)); pos_ += (size_t)(e - p) + 1; return true; }
            out.append(p, len_ - pos_);
            pos_ = len_;
        }
    }
    gzFile f_;
    vector<char> buf_;
    size_t pos_ = 0, len_ = 0;
    bool done_ = false;
};

static void put(const string &s) { fwrite(s.data(), 1, s.size(), stdout); }

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: see the source\n"); return 2; }
    const string cmd = argv[1];
    if (cmd == "isfastq") { printf("%d\n", mkhost::file_is_fastq(argv[2]) ? 1 : 0); return 0; }
    if (cmd == "records") {
        mkhost::RecordStream in(argv[2]);
        string h, r, q;
        printf("fastq %d\n", in.fastq() ? 1 : 0);
        while (in.record(h, r, &q)) { put(h); put("\t"); put(r); put("\t"); put(q); put("\n"); }
        if (!in.error.empty()) { put("error: " + in.error + "\n"); }
        return 0;
    }
    if (argc < 5) return 2;
    const uint32_t k = (uint32_t)atoi(argv[2]);
    if (cmd == "dump") {
        mkhost::RecordStream in(argv[4]);
        vector<string> h, s, q;
        printf("fastq %d\n", in.fastq() ? 1 : 0);
        while (in.next((size_t)atoi(argv[3]), k, h, s, &q)) {
            if (h.size() != s.size() || q.size() != s.size()) return 3;
            for (size_t i = 0; i < s.size(); ++i) { put(h[i]); put("\t"); put(s[i]); put("\t"); put(q[i]); put("\n"); }
        }
        if (!in.error.empty()) put("error: " + in.error + "\n");
        return 0;
    }
    if (cmd == "old") {
        mkhost::RecordStream in(argv[4]);
        OldRecordStream old(argv[4]);
        vector<string> h, s, oh, os;
        size_t n = 0;
        for (;;) {
            const bool a = in.next((size_t)atoi(argv[3]), k, h, s), b = old.next((size_t)atoi(argv[3]), k, oh, os);
            if (a != b || h != oh || s != os) { printf("differ after %zu records\n", n); return 0; }
            if (!a) break;
            n += s.size();
        }
        printf("same %zu\n", n);
        return 0;
    }
    if (cmd == "pairs" && argc >= 6) {
        mkhost::RecordStream in(argv[4]);
        mkhost::PairStream pairs(in, argv[4], argv[5]);
        if (argc > 6) pairs.max_bases = (uint64_t)atol(argv[6]);
        vector<string> h, a, b, qa, qb;
        while (pairs.next((size_t)atoi(argv[3]), k, h, a, b, &qa, &qb))
            for (size_t i = 0; i < a.size(); ++i) { put(h[i]); put("\t"); put(a[i]); put("\t"); put(b[i]); put("\t"); put(qa[i]); put("\t"); put(qb[i]); put("\n"); }
        if (!pairs.error.empty()) put("error: " + pairs.error + "\n");
        return 0;
    }
    if (cmd == "quality") {
        const uint32_t min_qual = (uint32_t)atoi(argv[3]);
        mkhost::QualityCount count;
        mkhost::RecordStream in(argv[4]);
        in.max_bases = mkhost::kQualityBasesMax;
        vector<string> h, a, b, qa, qb;
        if (argc >= 6) {
            mkhost::PairStream pairs(in, argv[4], argv[5]);
            pairs.max_bases = mkhost::kQualityBasesMax;
            while (pairs.next(1000, k, h, a, b, &qa, &qb))
                for (size_t i = 0; i < a.size(); ++i) count.pair(qa[i], qb[i], k, min_qual);
            if (!pairs.error.empty()) put("error: " + pairs.error + "\n");
        } else {
            while (in.next(1000, k, h, a, &qa))
                for (size_t i = 0; i < a.size(); ++i) count.read(qa[i], k, min_qual);
            if (!in.error.empty()) put("error: " + in.error + "\n");
        }
        put(count.line(min_qual) + "\n");
        return 0;
    }
    return 2;
}
