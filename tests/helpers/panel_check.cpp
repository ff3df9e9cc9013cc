// host/panel.hpp against a restatement that shares nothing with it (printf into a stream, the count from a separate loop), on
// seeded random counts of every small size and on the shapes a panel file has (nothing covered, everything covered, the largest
// values), the list reader on lines of every length -- built under AddressSanitizer + UBSan by tests/test_panel_abi.py.
// Prints "ok <cases>".
#include <cinttypes>
#include <cstdio>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "cover.hpp"
#include "panel.hpp"

static bool same(uint64_t sample, const std::vector<uint32_t> &cov, const std::vector<uint32_t> &ss, uint64_t queries, uint64_t cells, uint32_t h,
                 uint32_t fp_bits)
{
    std::ostringstream want;
    want << "kept";
    uint64_t genomes = 0;
    for (size_t j = 0; j < cov.size(); ++j) {
        if (cov[j] == 0) continue;
        char line[128];
        snprintf(line, sizeof line, "%" PRIu64 "\t%zu\t%" PRIu32 "\t%" PRIu32 "\n", sample, j, cov[j], ss[j]);
        want << line;
    }
    for (uint32_t x : cov) genomes += x != 0;
    std::string text = "kept";
    const uint64_t got = mkhost::format_panel(sample, cov.data(), ss.data(), cov.size(), text);
    if (text != want.str() || got != genomes) { printf("differs at n = %zu\n", cov.size()); return false; }
    // the sample's lines without their first field are the -C file's
    std::string cut, cover;
    const std::string first = std::to_string(sample) + "\t";
    for (size_t at = 4; at < text.size();) {
        const size_t end = text.find('\n', at) + 1;
        if (text.compare(at, first.size(), first) != 0) { printf("a line of another sample at n = %zu\n", cov.size()); return false; }
        cut += text.substr(at + first.size(), end - at - first.size());
        at = end;
    }
    if (mkhost::format_cover(cov.data(), ss.data(), cov.size(), cover) != genomes || cut != cover) { printf("not the cover file at n = %zu\n", cov.size()); return false; }
    char line[256];
    snprintf(line, sizeof line, "panel[%" PRIu64 "]: %" PRIu64 " queries, %" PRIu64 " of %" PRIu64 " cells seen, %" PRIu64 " genomes covered", sample, queries,
             cells, (uint64_t)1 << (h + fp_bits), genomes);
    if (mkhost::panel_sample_summary(sample, queries, cells, h, fp_bits, genomes) != line) { printf("summary differs at n = %zu\n", cov.size()); return false; }
    return true;
}

static bool list_ok()
{
    std::vector<std::string> files;
    mkhost::panel_list_files("", files);
    mkhost::panel_list_files("\n\n", files);
    mkhost::panel_list_files("abc\nab\n\n", files);                 // three characters do not count
    if (!files.empty()) return false;
    mkhost::panel_list_files("a.fa\n\nabc\nreads/b.fq\r\nlast", files);
    if (files != std::vector<std::string>{"a.fa", "reads/b.fq", "last"}) return false;
    files.clear();
    mkhost::panel_list_files("abc\r\nabcd", files);                 // (the carriage return is not a fourth character)
    return files == std::vector<std::string>{"abcd"};
}

int main()
{
    std::mt19937_64 rng(20263);
    unsigned cases = 0;
    for (uint32_t n = 0; n <= 70; ++n)
        for (int rep = 0; rep < 20; ++rep, ++cases) {
            std::vector<uint32_t> cov(n), ss(n);
            for (uint32_t j = 0; j < n; ++j) {
                ss[j] = (uint32_t)(rng() % 140000);
                cov[j] = rng() % 3 && ss[j] ? (uint32_t)(rng() % (ss[j] + 1)) : 0;
            }
            const uint32_t h = 1 + (uint32_t)(rng() % 28), bits = rng() % 2 ? 8 : 16;
            if (!same(rng() % 1000, cov, ss, rng() % 100000, rng() % ((uint64_t)1 << (h + bits)), h, bits)) return 1;
        }
    for (uint32_t n : {1u, 304u, 5000u}) {
        std::vector<uint32_t> none(n, 0), all(n, 131072), ss(n, 131072);
        if (!same(0, none, ss, 0, 0, 17, 8) || !same(95, all, ss, 3ull * n, (uint64_t)1 << 25, 17, 8)) return 1;
        cases += 2;
    }
    {   // the largest values there are: 2^28 partitions of 16-bit fingerprints, counts at the top of 32 bits
        std::vector<uint32_t> cov{UINT32_MAX, 0, 1u << 28}, ss{UINT32_MAX, UINT32_MAX, 1u << 28};
        if (!same(UINT64_MAX, cov, ss, UINT64_MAX, (uint64_t)1 << 44, 28, 16)) return 1;
        ++cases;
    }
    for (uint64_t n : {0ull, 1ull, 7ull, 8ull, 9ull, 16ull, 17ull, 96ull, 1000003ull}) {
        char line[128];
        snprintf(line, sizeof line, "panel: %" PRIu64 " samples, %" PRIu64 " passes over the matrix", n, (n + 7) / 8);
        if (mkhost::panel_summary(n, 8) != line) { printf("the last line differs at %" PRIu64 " samples\n", n); return 1; }
        ++cases;
    }
    if (!list_ok()) { printf("the list reader differs\n"); return 1; }
    ++cases;
    printf("ok %u\n", cases);
    return 0;
}
