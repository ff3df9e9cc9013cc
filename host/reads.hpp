// The read files of `miekki -a`, `-2` and `-S`: records streamed from a plain or gzip'd file.
// A file whose first byte, after inflation, is '@' and whose third line starts with '+' is FASTQ (the third line tells it from a
// 2-line file whose head lines happen to start with '@', which is read as it always was): a record is four lines -- the head,
// the sequence, a line that starts with '+', the quality string, as long as the sequence (Sanger / Illumina 1.8+, phred + 33).
// Multi-line FASTQ is not read.  A trailing partial record, a later record's third line that does not start with '+' and a
// quality line of another length than the sequence's are errors: `error` names the file and the record's ordinal (from 0,
// every record of the file counted), and nothing more is read.  The head line is handed out as it stands, '@' included.
// Anything else is read as strict 2-line records, as the reference's query_file does (Miekki.cpp:458-464): a head line, a
// sequence line, whatever they hold.
// With a quality threshold (-q), base j of a read is good when qual[j] >= 33 + min_qual, and the library cuts the read at
// its bad bases (mk_qset_upload_reads); what this header adds is the count the run prints: QualityCount.
// Plain C++ and zlib, no GPU in it.
#pragma once
#include <zlib.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace mkhost {

constexpr uint64_t kQualityBasesMax = 4096;                      // a read or pair with qualities (mk_qset_upload_reads' limit)

// `quality: <bad> of <bases> bases below <q>, <n> of <queries> queries without a k-mer left`: a query is a read or a pair; it
// has a k-mer left when some mate holds a stretch of k + 1 good bases
struct QualityCount {
    uint64_t bad = 0, bases = 0, queries = 0, none = 0;
    // one mate: its bases into the sums; true when it has a stretch of k + 1 good bases
    bool mate(const std::string &qual, uint32_t k, uint32_t min_qual)
    {
        uint64_t run = 0, best = 0;
        for (unsigned char c : qual) {
            if (c >= 33u + min_qual) { if (++run > best) best = run; }
            else { ++bad; run = 0; }
        }
        bases += qual.size();
        return best > k;
    }
    void read(const std::string &qual, uint32_t k, uint32_t min_qual)
    {
        ++queries;
        if (!mate(qual, k, min_qual)) ++none;
    }
    void pair(const std::string &qual1, const std::string &qual2, uint32_t k, uint32_t min_qual)
    {
        ++queries;
        const bool a = mate(qual1, k, min_qual), b = mate(qual2, k, min_qual);
        if (!a && !b) ++none;
    }
    std::string line(uint32_t min_qual) const
    {
        return "quality: " + std::to_string(bad) + " of " + std::to_string(bases) + " bases below " + std::to_string(min_qual) + ", " +
               std::to_string(none) + " of " + std::to_string(queries) + " queries without a k-mer left";
    }
};

class RecordStream {
public:
    explicit RecordStream(const std::string &path) : name_(path), f_(gzopen(path.c_str(), "rb")), buf_(4u << 20)
    {
        if (f_) gzbuffer(f_, 1u << 20);
        fill();                                                  // (the first buffer tells the format)
        if (len_ > 0 && buf_[0] == '@') {
            const char *b = buf_.data(), *e = b + len_;
            const char *l2 = (const char *)memchr(b, '\n', len_);
            const char *l3 = l2 ? (const char *)memchr(l2 + 1, '\n', (size_t)(e - (l2 + 1))) : nullptr;
            fastq_ = l3 && l3 + 1 < e && l3[1] == '+';
        }
    }
    ~RecordStream() { if (f_) gzclose(f_); }
    RecordStream(const RecordStream &) = delete;
    RecordStream &operator=(const RecordStream &) = delete;
    bool fastq() const { return fastq_; }
    const std::string &name() const { return name_; }
    std::string error;                                           // a FASTQ format error or a read beyond max_bases
    uint64_t max_bases = 0;                                      // next(): a kept read with more bases is an error (0: any length)
    // up to `want` records with at least k bases (shorter ones are dropped, 465-468); false at the end.  quals (FASTQ only):
    // the kept records' quality strings.
    bool next(size_t want, uint32_t k, std::vector<std::string> &heads, std::vector<std::string> &seqs, std::vector<std::string> *quals = nullptr)
    {
        heads.clear(); seqs.clear();
        if (quals) quals->clear();
        std::string head, ref, qual;
        while (seqs.size() < want && !done_ && error.empty()) {
            if (!record(head, ref, &qual)) break;
            if (ref.size() >= k) {
                if (max_bases && ref.size() > max_bases) {
                    error = "-q: read " + std::to_string(kept_) + " (" + head + ") of " + name_ + " holds " + std::to_string(ref.size()) +
                            " bases, more than the " + std::to_string(max_bases) + " a read with qualities may hold";
                    break;
                }
                ++kept_;
                heads.push_back(std::move(head)); seqs.push_back(std::move(ref));
                if (quals) quals->push_back(std::move(qual));
            }
            head.clear(); ref.clear(); qual.clear();
        }
        return !seqs.empty();
    }
    // the next record whatever its length; false when nothing was left, or on an error
    bool record(std::string &head, std::string &ref, std::string *qual = nullptr)
    {
        if (!error.empty()) return false;
        if (!fastq_) {
            const bool got_head = getline(head);
            const bool got_ref = getline(ref);
            if (qual) qual->clear();
            return got_head || got_ref;
        }
        std::string plus, q;
        if (!getline(head)) return false;
        const bool got_ref = getline(ref), got_plus = getline(plus), got_qual = getline(q);
        const std::string where = name_ + ": FASTQ record " + std::to_string(records_);
        if (!got_ref || !got_plus || !got_qual) error = where + " is cut short: a record is four lines";
        else if (plus.empty() || plus[0] != '+') error = where + ": its third line does not start with '+' (multi-line FASTQ is not read)";
        else if (q.size() != ref.size()) error = where + " has " + std::to_string(ref.size()) + " bases and " + std::to_string(q.size()) + " qualities";
        if (!error.empty()) { done_ = true; return false; }
        ++records_;
        if (qual) qual->swap(q);
        return true;
    }
private:
    void fill()
    {
        pos_ = len_ = 0;
        if (done_ || !f_) { done_ = true; return; }
        const int n = gzread(f_, buf_.data(), (unsigned)buf_.size());
        if (n <= 0) { done_ = true; return; }
        len_ = (size_t)n;
    }
    bool getline(std::string &out)                               // std::getline: false only when nothing was left
    {
        out.clear();
        bool any = false;
        for (;;) {
            if (pos_ == len_) {
                if (done_) return any;
                fill();
                if (done_) return any;
            }
            any = true;
            const char *p = buf_.data() + pos_;
            const char *e = (const char *)memchr(p, '\n', len_ - pos_);
            if (e) { out.append(p, (size_t)(e - p)); pos_ += (size_t)(e - p) + 1; return true; }
            out.append(p, len_ - pos_);
            pos_ = len_;
        }
    }
    std::string name_;
    gzFile f_;
    std::vector<char> buf_;
    size_t pos_ = 0, len_ = 0;
    bool done_ = false, fastq_ = false;
    uint64_t records_ = 0, kept_ = 0;                            // FASTQ records read; records next() kept
};

// what a RecordStream over the (plain or gzip'd) file would read it as
inline bool file_is_fastq(const std::string &path) { return RecordStream(path).fastq(); }

// -2: the records of two files in step, the i-th of one with the i-th of the other -- header lines are not compared.  A
// pair is kept when at least one mate has at least k bases (the record rule of 465-468 applied to the pair).  `error`
// is set, and nothing more is read, when one file ends before the other, a file has a format error, or a pair holds more
// k-mers than a pair may (max_bases: more bases than a pair with qualities may).
constexpr uint64_t kPairKmersMax = 4096;                         // (mk_qset_upload_pairs' limit)
class PairStream {
public:
    PairStream(RecordStream &first, const std::string &first_name, const std::string &second_name)
        : a_(first), b_(second_name), name_a_(first_name), name_b_(second_name) {}
    std::string error;
    uint64_t max_bases = 0;
    bool second_is_fastq() const { return b_.fastq(); }
    bool next(size_t want, uint32_t k, std::vector<std::string> &heads, std::vector<std::string> &seqs1, std::vector<std::string> &seqs2,
              std::vector<std::string> *quals1 = nullptr, std::vector<std::string> *quals2 = nullptr)
    {
        heads.clear(); seqs1.clear(); seqs2.clear();
        if (quals1) quals1->clear();
        if (quals2) quals2->clear();
        std::string h1, r1, h2, r2, q1, q2;
        while (seqs1.size() < want && error.empty()) {
            const bool got1 = a_.record(h1, r1, &q1), got2 = b_.record(h2, r2, &q2);
            if (!a_.error.empty() || !b_.error.empty()) { error = a_.error.empty() ? b_.error : a_.error; break; }
            if (!got1 && !got2) break;
            if (got1 != got2) {
                error = "-2: " + (got1 ? name_b_ : name_a_) + " ends after " + std::to_string(records_) + " records, before " +
                        (got1 ? name_a_ : name_b_) + " does: the two files pair record by record";
                break;
            }
            ++records_;
            if (r1.size() < k && r2.size() < k) continue;
            const uint64_t nk = (r1.size() > k ? r1.size() - k : 0) + (r2.size() > k ? r2.size() - k : 0);
            if (max_bases && r1.size() + r2.size() > max_bases) {
                error = "-q: pair " + std::to_string(run_) + " (" + h1 + ") holds " + std::to_string(r1.size() + r2.size()) + " bases, more than the " +
                        std::to_string(max_bases) + " a pair with qualities may hold";
                break;
            }
            if (nk > kPairKmersMax) {
                error = "-2: pair " + std::to_string(run_) + " (" + h1 + ") holds " + std::to_string(nk) + " k-mers, more than the " +
                        std::to_string(kPairKmersMax) + " a read pair may hold: read pairs are short reads";
                break;
            }
            ++run_;
            heads.push_back(std::move(h1)); seqs1.push_back(std::move(r1)); seqs2.push_back(std::move(r2));
            if (quals1) quals1->push_back(std::move(q1));
            if (quals2) quals2->push_back(std::move(q2));
        }
        return !seqs1.empty();
    }
private:
    RecordStream &a_;
    RecordStream b_;
    std::string name_a_, name_b_;
    size_t records_ = 0, run_ = 0;                               // records read from each file; pairs kept (-Y's ordinals)
};

}  // namespace mkhost
