// The files of `miekki -T <taxonomy> -y <report> [-Y <per read>] [-m <margin>]`: reads placed in a taxonomy by lowest common
// ancestor (mk_qset_run_lca).
// -T has one node per line, `<first_id> <last_id> [name]`: decimal ids, both inclusive, separated by blanks or tabs, the name
// the rest of the line; blank lines and lines that start with # are ignored.  The nodes are nested intervals in PREORDER: a
// parent before its children, by ascending first id (among equal first ids the larger last id first); a node's number is its
// position among the nodes.  Genomes inside no node are left out of the pass.
// -y gets one line per node whose subtree holds at least one read, in node order:
// <node> TAB <depth> TAB <first_id> TAB <last_id> TAB <clade_reads> TAB <reads> TAB <best_matches> TAB <hits> TAB <name>,
// roots at depth 0, clade_reads = the reads of the node and of everything below it.
// -Y gets one line per record that is run: <ordinal> TAB <node>, the node a number, * for above every node, - for unassigned.
// `miekki -T <taxonomy> -U <file>`: the distinct covered cells per node (mk_taxonomy_cover).  -U gets one line per node with
// covered > 0, in node order: <node> TAB <depth> TAB <first_id> TAB <last_id> TAB <covered> TAB <held> TAB <name>.
// `miekki -T <taxonomy> -V <file>`: the taxon-specific cells (mk_taxonomy_markers).  -V gets one line per node whose subtree has a
// covered cell, in node order: <node> TAB <depth> TAB <first_id> TAB <last_id> TAB <clade_covered> TAB <clade_specific> TAB
// <covered> TAB <specific> TAB <name>, clade_* = the node's and everything below it.
// Plain C++, no GPU in it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "miekki_hip.h"

namespace mkhost {

struct Taxonomy {
    std::vector<uint32_t> lo, hi;        // per node: [lo, hi), as mk_taxonomy_create takes them
    std::vector<uint32_t> parent, depth; // per node: the smallest enclosing node or MK_NO_NODE, the number of ancestors
    std::vector<std::string> name;
    std::vector<uint64_t> line;          // per node: its line in the file
};

// `text` = the file's bytes, `name` = what the messages call it.  False (and why, with the line) for a line that is not two ids,
// a last id below the first, a node equal to an earlier one, one that overlaps another without lying inside it, and an order
// other than preorder.  A file without nodes is a taxonomy without nodes.
inline bool parse_taxonomy(const std::string &text, const std::string &name, Taxonomy &out, std::string &why)
{
    out = Taxonomy();
    std::vector<uint32_t> open;                                  // the nodes that contain the current one's first id, outermost first
    uint64_t line_no = 0;
    auto blank = [](char ch) { return ch == ' ' || ch == '\t' || ch == '\r' || ch == '\v' || ch == '\f'; };
    for (size_t at = 0; at < text.size();) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        ++line_no;
        size_t b = at, e = end;
        while (b < e && blank(text[b])) ++b;
        while (e > b && blank(text[e - 1])) --e;
        at = end + 1;
        if (b == e || text[b] == '#') continue;
        const std::string where = "-T: line " + std::to_string(line_no) + " of " + name;
        uint64_t id[2] = {0, 0};
        bool ok = true;
        for (int f = 0; f < 2 && ok; ++f) {
            const size_t d0 = b;
            while (b < e && text[b] >= '0' && text[b] <= '9' && b - d0 < 10) id[f] = id[f] * 10 + (uint64_t)(text[b++] - '0');
            ok = b > d0 && (b == e || blank(text[b])) && id[f] < 0xfffffffeull && (f == 1 || b < e);
            while (b < e && blank(text[b])) ++b;
        }
        if (!ok) { why = where + " is not a node, <first_id> <last_id> [name]"; return false; }
        if (id[1] < id[0]) { why = where + ": the last id " + std::to_string(id[1]) + " is below the first, " + std::to_string(id[0]); return false; }
        const uint32_t lo = (uint32_t)id[0], hi = (uint32_t)id[1] + 1;
        const size_t v = out.lo.size();
        auto shown = [&](size_t u) { return "node " + std::to_string(u) + " (line " + std::to_string(out.line[u]) + ", " + std::to_string(out.lo[u]) + " " + std::to_string(out.hi[u] - 1) + ")"; };
        if (v && lo == out.lo[v - 1] && hi == out.hi[v - 1]) { why = where + ": the node repeats " + shown(v - 1); return false; }
        if (v && (lo < out.lo[v - 1] || (lo == out.lo[v - 1] && hi > out.hi[v - 1]))) {
            why = where + ": the node comes after " + shown(v - 1) + ": the nodes are not in preorder (a parent before its children, by ascending first id)";
            return false;
        }
        while (!open.empty() && out.hi[open.back()] <= lo) open.pop_back();
        if (!open.empty() && hi > out.hi[open.back()]) { why = where + ": the node overlaps " + shown(open.back()) + " without lying inside it"; return false; }
        out.lo.push_back(lo); out.hi.push_back(hi);
        out.parent.push_back(open.empty() ? MK_NO_NODE : open.back());
        out.depth.push_back((uint32_t)open.size());
        out.name.push_back(text.substr(b, e - b));
        out.line.push_back(line_no);
        open.push_back((uint32_t)v);
    }
    return true;
}

// False (and why) for a node that reaches beyond the index
inline bool taxonomy_fits(const Taxonomy &t, const std::string &name, uint64_t n_genomes, std::string &why)
{
    for (size_t v = 0; v < t.lo.size(); ++v)
        if (t.hi[v] > n_genomes) {
            why = "-T: line " + std::to_string(t.line[v]) + " of " + name + ": genome id " + std::to_string(t.hi[v] - 1) + " is beyond the index's " +
                  std::to_string(n_genomes) + " genomes";
            return false;
        }
    return true;
}

struct LcaCounts {
    uint64_t assigned = 0, above = 0, nodes = 0;   // reads over all slots, the last slot's, nodes with reads of their own
};

// lt[v] = the counters of node v, lt[n_nodes] those of "above every node"; `text` is appended to
inline void format_lca_report(const mk_lca_tally *lt, const Taxonomy &t, std::string &text, LcaCounts &counts)
{
    const size_t n = t.lo.size();
    counts = LcaCounts();
    std::vector<uint64_t> clade(n);
    for (size_t v = 0; v < n; ++v) clade[v] = lt[v].reads;
    for (size_t v = n; v-- > 0;)
        if (t.parent[v] != MK_NO_NODE) clade[t.parent[v]] += clade[v];     // (preorder: a child after its parent)
    for (size_t v = 0; v < n; ++v) {
        counts.assigned += lt[v].reads;
        counts.nodes += lt[v].reads != 0;
        if (!clade[v]) continue;
        text += std::to_string(v); text += '\t';
        text += std::to_string(t.depth[v]); text += '\t';
        text += std::to_string(t.lo[v]); text += '\t';
        text += std::to_string(t.hi[v] - 1); text += '\t';
        text += std::to_string(clade[v]); text += '\t';
        text += std::to_string(lt[v].reads); text += '\t';
        text += std::to_string(lt[v].best_matches); text += '\t';
        text += std::to_string(lt[v].hits); text += '\t';
        text += t.name[v]; text += '\n';
    }
    counts.above = lt[n].reads;
    counts.assigned += counts.above;
}

// the -Y lines of `n` records whose first has the ordinal `first`; `text` is appended to
inline void format_lca_reads(const uint32_t *node, uint64_t n, uint64_t first, std::string &text)
{
    for (uint64_t i = 0; i < n; ++i) {
        text += std::to_string(first + i); text += '\t';
        if (node[i] == MK_NO_NODE) text += '-';
        else if (node[i] == MK_LCA_ABOVE) text += '*';
        else text += std::to_string(node[i]);
        text += '\n';
    }
}

// -U: nc[v] = held and covered of node v; a line per node with covered > 0, in node order; `text` is appended to.  Returns the
// number of such nodes.
inline uint64_t format_taxon_cover(const mk_node_cover *nc, const Taxonomy &t, std::string &text)
{
    uint64_t nodes = 0;
    for (size_t v = 0; v < t.lo.size(); ++v) {
        if (!nc[v].covered) continue;
        ++nodes;
        text += std::to_string(v); text += '\t';
        text += std::to_string(t.depth[v]); text += '\t';
        text += std::to_string(t.lo[v]); text += '\t';
        text += std::to_string(t.hi[v] - 1); text += '\t';
        text += std::to_string(nc[v].covered); text += '\t';
        text += std::to_string(nc[v].held); text += '\t';
        text += t.name[v]; text += '\n';
    }
    return nodes;
}

inline std::string taxon_cover_summary(uint64_t queries, uint64_t cells, uint32_t h, uint32_t fp_bits, uint64_t covered_nodes, uint64_t nodes)
{
    return "taxon cover: " + std::to_string(queries) + " queries, " + std::to_string(cells) + " of " + std::to_string(1ull << (h + fp_bits)) +
           " cells seen, " + std::to_string(covered_nodes) + " of " + std::to_string(nodes) + " nodes covered";
}

// -V: nm[v] = specific and covered of node v, nm[nodes] of the slot above every node; a line per node whose subtree has a
// covered cell, in node order; `text` is appended to.  The subtree sums are made here, children before parents: the nodes are
// in preorder.  Returns what the summary line says.
struct MarkerCounts { uint64_t specific = 0, covered = 0, covered_nodes = 0, nodes = 0, above_specific = 0, above_covered = 0; };
inline MarkerCounts format_markers(const mk_node_markers *nm, const Taxonomy &t, std::string &text)
{
    const size_t n = t.lo.size();
    std::vector<uint64_t> clade_specific(n), clade_covered(n);
    MarkerCounts c;
    c.nodes = n;
    c.above_specific = nm[n].specific;
    c.above_covered = nm[n].covered;
    for (size_t v = n; v-- > 0;) {
        clade_specific[v] += nm[v].specific;
        clade_covered[v] += nm[v].covered;
        c.specific += nm[v].specific;
        c.covered += nm[v].covered;
        if (t.parent[v] != MK_NO_NODE) {
            clade_specific[t.parent[v]] += clade_specific[v];
            clade_covered[t.parent[v]] += clade_covered[v];
        }
    }
    for (size_t v = 0; v < n; ++v) {
        if (!clade_covered[v]) continue;
        ++c.covered_nodes;
        text += std::to_string(v); text += '\t';
        text += std::to_string(t.depth[v]); text += '\t';
        text += std::to_string(t.lo[v]); text += '\t';
        text += std::to_string(t.hi[v] - 1); text += '\t';
        text += std::to_string(clade_covered[v]); text += '\t';
        text += std::to_string(clade_specific[v]); text += '\t';
        text += std::to_string(nm[v].covered); text += '\t';
        text += std::to_string(nm[v].specific); text += '\t';
        text += t.name[v]; text += '\n';
    }
    return c;
}

inline std::string markers_summary(uint64_t queries, const MarkerCounts &c)
{
    return "markers: " + std::to_string(queries) + " queries, " + std::to_string(c.covered) + " of " + std::to_string(c.specific) +
           " specific cells covered, " + std::to_string(c.covered_nodes) + " of " + std::to_string(c.nodes) + " nodes covered, " +
           std::to_string(c.above_covered) + " of " + std::to_string(c.above_specific) + " cells above every node";
}

inline std::string lca_summary(uint64_t queries, const LcaCounts &c, uint32_t margin)
{
    return "lca: " + std::to_string(queries) + " queries, " + std::to_string(c.assigned) + " assigned, " + std::to_string(c.above) +
           " above every node, " + std::to_string(c.nodes) + " nodes with reads, margin " + std::to_string(margin);
}

}  // namespace mkhost
