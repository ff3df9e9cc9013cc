// Small text files of the command line (lists, -K / -L / -T files, 2-line records): whether a file is there, its
// whole text, its lines.  Plain zlib, nothing of the library: what host/options.hpp needs links without it.
#pragma once
#include <sys/stat.h>
#include <zlib.h>

#include <string>
#include <vector>

namespace mkhost {

inline bool file_exists(const std::string &path)
{
    struct stat st;
    return stat(path.c_str(), &st) == 0;
}

// whole file; gunzipped when it carries the gzip magic (zstr.hpp:157-167 semantics)
inline bool read_text(const std::string &path, std::string &out)
{
    gzFile f = gzopen(path.c_str(), "rb");          // transparent for non-gzip input
    if (!f) return false;
    gzbuffer(f, 1 << 20);
    out.clear();
    std::vector<char> buf(1 << 20);
    int n;
    while ((n = gzread(f, buf.data(), (unsigned)buf.size())) > 0) out.append(buf.data(), (size_t)n);
    gzclose(f);
    return n == 0;
}

inline std::vector<std::string> split_lines(const std::string &text)   // getline semantics
{
    std::vector<std::string> lines;
    size_t pos = 0;
    while (pos <= text.size()) {
        size_t e = text.find('\n', pos);
        if (e == std::string::npos) e = text.size();
        lines.emplace_back(text, pos, e - pos);
        pos = e + 1;
    }
    return lines;
}

}  // namespace mkhost
