// The outputs of the `miekki` binary that sum the reads of -a, or of -S's samples, on the device instead of listing them;
// none of these flags is in the reference:
//   * -P <file> with -a (not in the reference): the profile of the read set instead of a line per read -- per genome, how many
//     reads list it, list it alone, have it as their best hit -- summed on the device (profile_file below).  One GPU.
//   * -L <file> -p <file> with -a (not in the reference): the same profile by CLADE -- -L groups the indexed genomes in -F's
//     layout, -p gets per clade the reads that list a member (once each), list no other clade, have their best hit in it
//     (mk_qset_run_clade_tally; host/clades.hpp).  Genomes -L does not name are left out of the pass.  Alone or beside -P
//     (one scan serves both) and the flags below.  One GPU.
//   * -T <file> -y <file> [-Y <file>] [-m <margin>] with -a (not in the reference): every read placed in a taxonomy by lowest
//     common ancestor -- -T holds nested intervals of genome ids in preorder, -y gets per node the reads whose hits it is the
//     deepest node to hold, with subtree sums, -Y each read's node (mk_qset_run_lca; host/taxonomy.hpp).  Genomes inside no
//     node are left out of the pass.  Alone or beside the flags around it, with a scan of its own.  One GPU.
//   * -T <file> -U <file> with -a (not in the reference; KrakenUniq's unique k-mer counts): per node of the taxonomy the distinct
//     cells its genomes hold and those of them the read set's gated sketches hold (mk_taxonomy_cover; host/taxonomy.hpp) over
//     the table that -C, -W and -G mark, marked once.  Alone or beside -y and every flag around it.  One GPU.
//   * -T <file> -V <file> with -a (not in the reference; Kraken's k-mer LCA, MetaPhlAn's clade markers): every held cell belongs
//     to the deepest node that contains all its holders; per node the cells it owns and those of them the read set's gated
//     sketches hold, with subtree sums (mk_taxonomy_markers; host/taxonomy.hpp), over the same table, at the end.  One GPU.
//   * -C <file> with -a (not in the reference): breadth of coverage -- per genome, how many of its stored fingerprints the read
//     set's gated sketches hold (mk_qset_run_cover, mk_cover_count; profile_file below).  Alone or beside -P.  One GPU.
//   * -W <file> with -a (not in the reference; Mash screen's -w): the winner-takes-all screen -- every cell the read set marks is
//     credited to ONE genome, the best-contained of its holders, and each genome reports the cells it wins (mk_cover_winners;
//     host/winners.hpp).  One round: the order comes from -C's plain counts.  Alone or beside -C and / or -P.  One GPU.
//   * -S <list> -c <file> (not in the reference): the cover of a cohort -- the list names read files, one sample each; eight
//     samples share one table and one pass over the matrix (mk_qset_run_panel, mk_panel_count; panel_files below; host/panel.hpp).
//     No -a.  One GPU.
//   * -D <file> with -a (not in the reference; Mash screen's median multiplicity): depth of coverage -- per genome, over its
//     stored fingerprints that the read set holds, in how many reads each turns up: the lower median and the sum
//     (mk_qset_run_depth, mk_depth_profile; host/depth.hpp).  Alone or beside -P, -C and -W.  One GPU.
//   * -G <file> with -a, -g <int> (not in the reference; sourmash's gather): the greedy set cover over -C's table -- the genome
//     that explains most of what is still unexplained, its cells struck, and again until no genome explains -g (10) cells: one
//     line per pick, in pick order (mk_cover_gather; host/gather.hpp).  Alone or beside -P, -C, -W and -D.  One GPU.
//   * -E <file> with -a, -I <int>, -w <int> (not in the reference; the EM of Kallisto, Salmon, Centrifuge): abundance -- how many
//     reads each genome gets when a read that several genomes share (those within -w percent of its best one, default 100) is
//     split among them in proportion to what the other reads say, -I (50) times (mk_qset_run_share, mk_share_rounds;
//     host/abundance.hpp).  Alone or beside every flag above, with a scan of its own.  One GPU.
#include "driver.hpp"

#include <algorithm>

#include "abundance.hpp"
#include "cover.hpp"
#include "depth.hpp"
#include "gather.hpp"
#include "panel.hpp"
#include "profile.hpp"
#include "winners.hpp"

using namespace std;

namespace mkhost {

namespace {

using ProfileJob = Driver::ProfileJob;
constexpr size_t kSuperBatch = Driver::kSuperBatch;

// ---- -P -p -y -U -V -C -W -D -G -E: query_file's reads -- the same records, super-batches and marks, the approximate mode's thresholds --
// summed on the device instead of listed per read (one context): counters and tables that are reset once, added to by every
// super-batch's passes, read once at the end.  A super-batch is read and uploaded once for all of them.  Nothing per read
// comes back but -Y's nodes; the -o file receives nothing.
void emit(const char *flag, const string &path, const string &text, const string &summary) { write_text(flag, path, text); cout << summary << endl; }

// the parameters and the sketch sizes that the cover, winners, depth and panel files are formatted with
bool index_sizes(mk_ctx *ctx, uint32_t G, mk_params &p, vector<uint32_t> &sketch)
{
    vector<uint64_t> sizes(G);
    sketch.resize(G);
    return mk_get_params(ctx, &p) == MK_OK && (!G || mk_index_export_sizes(ctx, sizes.data(), sketch.data()) == MK_OK);
}

// The outputs of a profile run, each with its device state and three steps: open (before the reads), run (queues one
// super-batch's pass), close (the read, the file, the summary line).  A step that fails dies under its own flag.
struct TallyOut {                                                         // -P
    void *d = nullptr;
    void open(const ProfileJob &j)
    {
        must(mk_dev_alloc(j.ctx, (uint64_t)std::max<uint32_t>(j.G, 1) * sizeof(mk_tally), &d), "-P: no room for the counters");
        must(mk_tally_reset(j.ctx, (mk_tally *)d, j.G), "-P: profile failed");
    }
    void run(const ProfileJob &j, mk_qset *qs) { must(mk_qset_run_tally(j.ctx, qs, 10, j.min_inter, (mk_tally *)d, j.G), "-P: profile failed"); }   // (Miekki.cpp:437's thresholds)
    void close(const ProfileJob &j)
    {
        vector<mk_tally> tally(j.G);
        must(mk_tally_read(j.ctx, (const mk_tally *)d, j.G, tally.data()), "-P: profile failed");
        mk_dev_free(j.ctx, d);
        string text;
        mkhost::ProfileCounts counts;
        mkhost::format_profile(tally.data(), tally.size(), text, counts);
        emit("-P", j.tally_path, text, mkhost::profile_summary(j.done, counts));
    }
};
struct CladeOut {                                                         // -L -p
    void *d = nullptr;
    mk_clade_map *map = nullptr;
    uint32_t n = 0;
    void open(const ProfileJob &j)
    {
        vector<uint32_t> ids;                                             // (an id beyond the index is refused here: before the reads are opened)
        string why;
        if (!mkhost::clade_map_of(*j.clades, j.G, ids, why)) { cout << why << endl; exit(1); }
        must(mk_clade_map_create(j.ctx, ids.data(), j.G, &map), "-p: the clade map was refused");
        n = mk_clade_map_size(map);
        must(mk_dev_alloc(j.ctx, (uint64_t)std::max<uint32_t>(n, 1) * sizeof(mk_clade_tally), &d), "-p: no room for the counters");
        must(mk_clade_tally_reset(j.ctx, (mk_clade_tally *)d, n), "-p: profile failed");
    }
    // d_tally: null, or -P's counters, which the same scan then adds to
    void run(const ProfileJob &j, mk_qset *qs, void *d_tally)
    {
        must(mk_qset_run_clade_tally(j.ctx, qs, 10, j.min_inter, map, (mk_clade_tally *)d, n, (mk_tally *)d_tally, j.G), "-p: profile failed");
    }
    void close(const ProfileJob &j)
    {
        vector<mk_clade_tally> ct(n);
        must(mk_clade_tally_read(j.ctx, (const mk_clade_tally *)d, n, ct.data()), "-p: profile failed");
        mk_dev_free(j.ctx, d);
        mk_clade_map_free(j.ctx, map);
        string text;
        mkhost::CladeCounts counts;
        mkhost::format_clade_profile(ct.data(), j.clades->first_id.data(), j.clades->members.data(), ct.size(), text, counts);
        emit("-p", j.clade_path, text, mkhost::clade_summary(j.done, counts));
    }
};
struct LcaOut {                                                           // -T -y -Y -m
    void *d = nullptr, *d_node = nullptr;                                 // the counters; with -Y, room for a super-batch's nodes
    mk_taxonomy *taxonomy = nullptr;
    uint32_t n_slots = 0;
    string node_text;
    vector<uint32_t> nodes;
    size_t run_before = 0;                                                // the records of the super-batches before this one
    void open(const ProfileJob &j)
    {
        string why;                                                       // (an id beyond the index is refused here: before the reads are opened)
        if (!mkhost::taxonomy_fits(*j.tax, j.tax_name, j.G, why)) { cout << why << endl; exit(1); }
        n_slots = (uint32_t)j.tax->lo.size() + 1;
        must(mk_taxonomy_create(j.ctx, j.tax->lo.data(), j.tax->hi.data(), n_slots - 1, j.G, &taxonomy), "-T: the taxonomy was refused");
        must(mk_dev_alloc(j.ctx, (uint64_t)n_slots * sizeof(mk_lca_tally), &d), "-y: no room for the counters");
        must(mk_lca_tally_reset(j.ctx, (mk_lca_tally *)d, n_slots), "-y: lca failed");
        if (!j.nodes_path.empty()) must(mk_dev_alloc(j.ctx, kSuperBatch * sizeof(uint32_t), &d_node), "-Y: no room for the nodes");
    }
    // a pass of its own; with -Y the batch's n nodes come back after it, the only thing per read that does
    void run(const ProfileJob &j, mk_qset *qs, size_t n)
    {
        if (d_node && n > kSuperBatch) die("-Y: a super-batch beyond the nodes' room");
        must(mk_qset_run_lca(j.ctx, qs, 10, j.min_inter, j.margin, taxonomy, (mk_lca_tally *)d, n_slots, (uint32_t *)d_node), "-y: lca failed");
        if (d_node && n) {
            nodes.resize(n);
            must(mk_dev_download(j.ctx, nodes.data(), d_node, n * sizeof(uint32_t)), "-Y: lca failed");
            mkhost::format_lca_reads(nodes.data(), nodes.size(), run_before, node_text);
        }
        run_before += n;
    }
    void close(const ProfileJob &j)
    {
        vector<mk_lca_tally> lt(n_slots);
        must(mk_lca_tally_read(j.ctx, (const mk_lca_tally *)d, n_slots, lt.data()), "-y: lca failed");
        mk_dev_free(j.ctx, d);
        if (d_node) mk_dev_free(j.ctx, d_node);
        mk_taxonomy_free(j.ctx, taxonomy);
        string text;
        mkhost::LcaCounts counts;
        mkhost::format_lca_report(lt.data(), *j.tax, text, counts);
        write_text("-y", j.lca_path, text);
        if (d_node) write_text("-Y", j.nodes_path, node_text);
        cout << mkhost::lca_summary(j.done, counts, j.margin) << endl;
    }
};
struct SeenOut {                                                          // the table of seen cells: -C, -W, -G, -U and -V read it
    void *d = nullptr;
    mk_taxonomy *taxonomy = nullptr;                                      // -U's and -V's
    string flag;                                                          // the first of -C -W -G -U -V that was given
    // the table goes after its last reader: -V, which runs at the end, or whoever calls this
    void free_table(const ProfileJob &j) { if (j.markers_path.empty()) mk_dev_free(j.ctx, d); }
    void open(const ProfileJob &j)
    {
        flag = !j.cover_path.empty() ? "-C" : !j.winners_path.empty() ? "-W" : !j.gather_path.empty() ? "-G" : !j.taxon_cover_path.empty() ? "-U" : "-V";
        must(mk_dev_alloc(j.ctx, mk_cover_bytes(j.ctx), &d), flag + ": no room for the table");
        must(mk_cover_reset(j.ctx, (uint32_t *)d), flag + ": cover failed");
    }
    void run(const ProfileJob &j, mk_qset *qs) { must(mk_qset_run_cover(j.ctx, qs, (uint32_t *)d), flag + ": cover failed"); }
    // -C and -W: with both, the count pass runs once and serves both files.  The table stays for -G.
    void close(const ProfileJob &j)
    {
        const bool want_winners = !j.winners_path.empty();
        vector<uint32_t> covered(j.G), won(j.G), sketch;
        uint64_t cells = 0, claimed = 0;
        mk_params p;
        const int rc = want_winners ? mk_cover_winners(j.ctx, (const uint32_t *)d, covered.data(), won.data(), &cells, &claimed)
                                    : mk_cover_count(j.ctx, (const uint32_t *)d, covered.data(), &cells);
        if (rc != MK_OK || !index_sizes(j.ctx, j.G, p, sketch)) die(flag + ": cover failed");
        if (j.gather_path.empty() && j.taxon_cover_path.empty()) free_table(j);
        string text;
        if (!j.cover_path.empty()) {
            const uint64_t genomes = mkhost::format_cover(covered.data(), sketch.data(), covered.size(), text);
            emit("-C", j.cover_path, text, mkhost::cover_summary(j.done, cells, p.h, p.fp_bits, genomes));
            text.clear();
        }
        if (want_winners) {
            const uint64_t genomes = mkhost::format_winners(won.data(), covered.data(), sketch.data(), j.G, text);
            emit("-W", j.winners_path, text, mkhost::winners_summary(j.done, claimed, cells, genomes));
        }
    }
    // -U, -V: the taxonomy is made (and an id beyond the index refused) before the reads are opened
    void open_taxonomy(const ProfileJob &j)
    {
        string why;
        if (!mkhost::taxonomy_fits(*j.tax, j.tax_name, j.G, why)) { cout << why << endl; exit(1); }
        must(mk_taxonomy_create(j.ctx, j.tax->lo.data(), j.tax->hi.data(), (uint32_t)j.tax->lo.size(), j.G, &taxonomy), "-T: the taxonomy was refused");
    }
    // -U, after -C and -W, before -G: the node pass over the table; `last`: nobody reads the table after it
    void taxon_cover(const ProfileJob &j, bool last)
    {
        vector<mk_node_cover> nc(j.tax->lo.size());
        uint64_t cells = 0;
        mk_params p;
        if (mk_taxonomy_cover(j.ctx, taxonomy, (const uint32_t *)d, nc.data(), &cells) != MK_OK || mk_get_params(j.ctx, &p) != MK_OK) die("-U: taxon cover failed");
        if (j.markers_path.empty()) mk_taxonomy_free(j.ctx, taxonomy);
        if (last) free_table(j);
        string text;
        const uint64_t nodes = mkhost::format_taxon_cover(nc.data(), *j.tax, text);
        emit("-U", j.taxon_cover_path, text, mkhost::taxon_cover_summary(j.done, cells, p.h, p.fp_bits, nodes, nc.size()));
    }
    // -V, at the end: the marker pass over the table, which goes here with the taxonomy
    void markers(const ProfileJob &j)
    {
        vector<mk_node_markers> nm(j.tax->lo.size() + 1);
        if (mk_taxonomy_markers(j.ctx, taxonomy, (const uint32_t *)d, nm.data(), (uint32_t)nm.size(), nullptr) != MK_OK) die("-V: markers failed");
        mk_taxonomy_free(j.ctx, taxonomy);
        mk_dev_free(j.ctx, d);
        string text;
        const mkhost::MarkerCounts counts = mkhost::format_markers(nm.data(), *j.tax, text);
        emit("-V", j.markers_path, text, mkhost::markers_summary(j.done, counts));
    }
    // -G, after everything else but -V: the greedy rounds over a copy of the table, with -D's table (d_mult, or null) for the fifth
    // field; both tables go here
    void gather(const ProfileJob &j, void *d_mult)
    {
        vector<mk_pick> picks(j.G);
        uint32_t n_picks = 0;
        uint64_t cells = 0, explained = 0;
        must(mk_cover_gather(j.ctx, (const uint32_t *)d, (const uint8_t *)d_mult, j.min_new, 0, picks.data(), &n_picks, &cells, &explained), "-G: gather failed");
        free_table(j);
        if (d_mult) mk_dev_free(j.ctx, d_mult);
        string text;
        mkhost::format_gather(picks.data(), n_picks, d_mult != nullptr, text);
        emit("-G", j.gather_path, text, mkhost::gather_summary(j.done, explained, cells, n_picks, j.min_new));
    }
};
struct DepthOut {                                                         // -D
    void *d = nullptr;
    void open(const ProfileJob &j)
    {
        must(mk_dev_alloc(j.ctx, mk_depth_bytes(j.ctx), &d), "-D: no room for the table");
        must(mk_depth_reset(j.ctx, (uint8_t *)d), "-D: depth failed");
    }
    void run(const ProfileJob &j, mk_qset *qs) { must(mk_qset_run_depth(j.ctx, qs, (uint8_t *)d), "-D: depth failed"); }
    void close(const ProfileJob &j)                                       // (the table stays for -G)
    {
        vector<mk_depth> depth(j.G);
        vector<uint32_t> sketch;
        uint64_t cells = 0, saturated = 0;
        mk_params p;
        if (mk_depth_profile(j.ctx, (const uint8_t *)d, depth.data(), &cells, &saturated) != MK_OK || !index_sizes(j.ctx, j.G, p, sketch)) die("-D: depth failed");
        if (j.gather_path.empty()) mk_dev_free(j.ctx, d);
        string text;
        const uint64_t genomes = mkhost::format_depth(depth.data(), sketch.data(), j.G, text);
        emit("-D", j.depth_path, text, mkhost::depth_summary(j.done, cells, saturated, p.h, p.fp_bits, genomes));
    }
};

struct AbundanceOut {                                                     // -E -I -w
    mk_sharepool *pool = nullptr;
    void open(const ProfileJob &j) { must(mk_share_create(j.ctx, &pool), "-E: no room for the pool"); }
    // a pass of its own
    void run(const ProfileJob &j, mk_qset *qs) { must(mk_qset_run_share(j.ctx, qs, 10, j.min_inter, j.share_margin, pool), "-E: abundance failed"); }
    void close(const ProfileJob &j)
    {
        vector<uint64_t> abundance(j.G), unique(j.G), shared(j.G);
        mk_share_info info;
        mk_share_result res;
        must(mk_share_rounds(j.ctx, pool, j.rounds, MK_SHARE_AUTO_SHIFT, abundance.data(), &res), "-E: abundance failed");
        must(mk_share_export(j.ctx, pool, unique.data(), shared.data(), nullptr, nullptr), "-E: abundance failed");
        must(mk_share_info_read(j.ctx, pool, &info), "-E: abundance failed");
        mk_share_free(j.ctx, pool);
        string text;
        const uint64_t genomes = mkhost::format_abundance(abundance.data(), unique.data(), shared.data(), j.G, 0, text);
        emit("-E", j.abundance_path, text, mkhost::abundance_summary(info, genomes, res, j.share_margin));
    }
};

// One super-batch as a set on the device for fn(qs), whose steps die under their own flags, and freed after it -- which
// waits for the passes fn queued.  The upload is a step too: `fail` is what it dies with.
template <class Fn>
void with_uploaded(Driver &drv, mk_ctx *ctx, const ReadBatch &b, const char *fail, Fn fn)
{
    mk_qset *qs = nullptr;
    // (-2: the batch's pairs as one query each, -q: cut at their bad bases -- every pass over the set is what it is for reads)
    drv.upload_batch(ctx, b, fail, &qs);
    fn(qs);
    mk_qset_free(ctx, qs);
}

}  // namespace

// The fixed sequence over the outputs: open, per super-batch the passes in the order tally or clades, cover, depth, lca,
// abundance -- one upload serves them all --, then the closes in the order of the summary lines.
void Driver::profile_file(ProfileJob j)
{
    j.ctx = ctx0(); j.G = group.total(); j.min_inter = 0.5 * threshold;
    const bool want_tally = !j.tally_path.empty(), want_clades = !j.clade_path.empty(), want_lca = !j.lca_path.empty();
    const bool want_gather = !j.gather_path.empty(), want_depth = !j.depth_path.empty();
    const bool want_taxon_cover = !j.taxon_cover_path.empty(), want_abundance = !j.abundance_path.empty();
    const bool want_markers = !j.markers_path.empty();
    const bool want_readers = !j.cover_path.empty() || !j.winners_path.empty(), want_seen = want_readers || want_gather || want_taxon_cover || want_markers;
    TallyOut tally;
    CladeOut clades;
    LcaOut lca;
    SeenOut seen;
    DepthOut depth;
    AbundanceOut abundance;
    if (want_clades) clades.open(j);
    if (want_lca) lca.open(j);
    if (want_taxon_cover || want_markers) seen.open_taxonomy(j);
    if (!mkhost::file_exists(j.reads)) { cout << "File problem" << endl; return; }
    if (want_tally) tally.open(j);
    if (want_seen) seen.open(j);
    if (want_depth) depth.open(j);
    if (want_abundance) abundance.open(j);
    j.done = for_read_batches(j.reads, [&](ReadBatch &b) {
        with_uploaded(*this, j.ctx, b, "-a: the upload failed", [&](mk_qset *qs) {   // (every pass is queued)
            if (want_clades) clades.run(j, qs, tally.d);                  // (with -P: its counters from the same scan)
            else if (want_tally) tally.run(j, qs);
            if (want_seen) seen.run(j, qs);
            if (want_depth) depth.run(j, qs);
            if (want_lca) lca.run(j, qs, b.q.size());
            if (want_abundance) abundance.run(j, qs);
        });
    });
    print_quality();
    if (want_tally) tally.close(j);
    if (want_clades) clades.close(j);
    if (want_lca) lca.close(j);
    if (want_readers) seen.close(j);
    if (want_depth) depth.close(j);
    if (want_taxon_cover) seen.taxon_cover(j, !want_gather);
    if (want_gather) seen.gather(j, depth.d);
    if (want_abundance) abundance.close(j);
    if (want_markers) seen.markers(j);
}

// ---- -S / -c: every listed file is a sample, read as -a reads one; the samples go in groups of eight through one table of
// (partition, value) bytes -- reset, every file's super-batches marked into its slot's bit (mk_qset_run_panel), one pass over
// the matrix for the group (mk_panel_count).  The -o file receives nothing.
void Driver::panel_files(const vector<string> &files, const string &out_path)
{
    mk_ctx *ctx = ctx0();
    const uint32_t G = group.total();
    void *d_panel = nullptr;
    mk_params p;
    vector<uint32_t> sketch;
    if (!index_sizes(ctx, G, p, sketch)) die("-S: panel failed");
    if (mk_dev_alloc(ctx, mk_panel_bytes(ctx), &d_panel) != MK_OK) die("-S: no room for the table");
    string text;
    for (size_t s0 = 0; s0 < files.size(); s0 += MK_PANEL_SLOTS) {
        const uint32_t n = (uint32_t)std::min<size_t>(MK_PANEL_SLOTS, files.size() - s0);
        if (mk_panel_reset(ctx, (uint8_t *)d_panel) != MK_OK) die("-S: panel failed");
        vector<size_t> done(n);
        for (uint32_t slot = 0; slot < n; ++slot)
            done[slot] = for_read_batches(files[s0 + slot], [&](ReadBatch &b) {
                with_uploaded(*this, ctx, b, "-S: panel failed", [&](mk_qset *qs) {
                    if (mk_qset_run_panel(ctx, qs, slot, (uint8_t *)d_panel) != MK_OK) die("-S: panel failed");             // (queued)
                });
            });
        vector<uint32_t> covered((size_t)n * G);
        vector<uint64_t> cells(n);
        if (mk_panel_count(ctx, (const uint8_t *)d_panel, n, covered.data(), cells.data()) != MK_OK) die("-S: panel failed");
        for (uint32_t slot = 0; slot < n; ++slot) {
            const uint64_t genomes = mkhost::format_panel(s0 + slot, covered.data() + (size_t)slot * G, sketch.data(), G, text);
            cout << mkhost::panel_sample_summary(s0 + slot, done[slot], cells[slot], p.h, p.fp_bits, genomes) << endl;
        }
    }
    mk_dev_free(ctx, d_panel);
    write_text("-c", out_path, text);
    print_quality();
    cout << mkhost::panel_summary(files.size(), MK_PANEL_SLOTS) << endl;
}

}  // namespace mkhost
