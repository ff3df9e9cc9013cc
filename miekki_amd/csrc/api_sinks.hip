// C ABI of libmiekki_hip.so, the sinks on the list walk and on a set's sketch: families (family.hip), tallies (tally.hip), clade
// tallies (clade.hip), lowest common ancestors (lca.hip), shared reads and their EM rounds (share.hip), cover and winners (cover.hip), taxon cover (taxcover.hip), taxon markers (markers.hip), depth (depth.hip), gather (gather.hip),
// representatives (rep.hip).  Host-side orchestration only, on api_query.hip's qset_leaves / qset_walk, for_uploaded_slices,
// for_index_sets and refuse_nan_lists (mk_internal.hpp).  What the counting sinks share stands once, before the first of them:
// their refusals, their counters' reset, read and one-shot use, and the per-genome map that a clade map and a taxonomy both are.
#include <algorithm>
#include <memory>

#include "cover_order.hpp"
#include "mk_internal.hpp"

using namespace mk;

// ---- what the sinks on the list walk share on the host ----------------------------------------------------------------------
// an array of one entry per genome id covers the ids the context reports; `what`: the array, for the message
static int refuse_ids_beyond(const mk_ctx *c, uint32_t n_ids, const char *what)
{
    if (!c->G || (uint64_t)c->p.genome_id_base + c->G <= n_ids) return MK_OK;
    set_error("the context reports genome ids up to %llu, beyond the %s's %u ids", (unsigned long long)c->p.genome_id_base + c->G - 1, what, n_ids);
    return MK_ERR_ARG;
}

// nothing to count: still the set's own checks, as a pass would make them -- a stale set from the index is MK_ERR_STATE
static int qset_checks_only(mk_ctx *c, mk_qset *qs) { return qset_leaves(c, qs, [](mk_qset *, const std::vector<uint32_t> *) { return MK_OK; }); }

// the body of the sinks' mk_*_read: the counters copied to the host, which waits for everything queued
template <typename T>
static int counters_read(mk_ctx *c, const T *d, uint32_t n, T *out)
{
    if (!c || (n && (!d || !out))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (n) MK_HIP(hipMemcpyAsync(out, d, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    return drain_timers(c);
}

// A one-shot mk_query_* call over uploaded sequences: n fresh counters, zeroed, added to by run(qs, q0, d) slice by slice (the
// sums do not depend on the slicing), then what last() queues, then read into `out` -- which waits, so the counters and
// whatever else the caller holds for the passes may go on return.
template <typename T, typename Run, typename Last = int (*)()>
static int query_counters(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t n, T *out, Run run, Last last = [] { return (int)MK_OK; })
{
    T *d = nullptr;
    MK_TRY(dev_alloc(&d, (uint64_t)n));
    DevGuard<T> guard(d);
    MK_TRY(counters_reset(c, d, n));
    MK_TRY(for_uploaded_slices(c, seqs, lens, nq, [&](mk_qset *qs, uint32_t q0, uint32_t) { return run(qs, q0, d); }));
    MK_TRY(last());
    return counters_read(c, d, n, out);
}

// One word per local genome on the device -- a clade number, a taxonomy's leaf -- padded to whole tiles with 0xffffffff ("left
// out": MK_NO_CLADE, MK_NO_NODE) as the size arrays are padded (the walk loads a lane's entries whole), and what the ids meant
// when it was made.  mk_clade_map and mk_taxonomy each hold one.
struct GenomeMap {
    const char *noun, *names;      // for the messages: "clade map", "entries"
    mk_ctx *owner = nullptr;
    uint32_t n = 0, padded = 0;    // genomes it was made for; entries of d_word: whole tiles of kTileBytes genomes
    uint32_t *d_word = nullptr;
    uint64_t index_id = 0;         // the context's index_id when it was made -- another value: the ids name other genomes
    GenomeMap(const GenomeMap &) = delete;                         // (with these mk_clade_map's and mk_taxonomy's copies)
    GenomeMap &operator=(const GenomeMap &) = delete;
    ~GenomeMap() { if (d_word) (void)hipFree(d_word); }
};

// word[n] padded and on the device when this returns (`upload` false: the fields only, nothing to walk)
static int genome_map_make(mk_ctx *c, GenomeMap &m, const uint32_t *word, uint32_t n, bool upload = true)
{
    m.owner = c; m.n = n; m.index_id = c->index_id;
    m.padded = (uint32_t)(((uint64_t)n + kTileBytes - 1) / kTileBytes * kTileBytes);   // (an index holds fewer than 0xffffff00 genomes)
    if (!m.padded || !upload) return MK_OK;
    std::vector<uint32_t> h(m.padded, 0xffffffffu);
    std::copy(word, word + n, h.begin());
    MK_TRY(dev_alloc(&m.d_word, (uint64_t)m.padded));
    MK_HIP(hipMemcpyAsync(m.d_word, h.data(), (size_t)m.padded * 4, hipMemcpyHostToDevice, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));                       // (from pageable memory that goes on return)
    return MK_OK;
}

// before a map goes: a queued pass may still read it
static void genome_map_wait(mk_ctx *c, const GenomeMap &m)
{
    mk_ctx *owner = c ? c : m.owner;
    if (owner && use_device(owner, false) == MK_OK) (void)hipStreamSynchronize(owner->stream);
}

// a pass's two refusals of a map, an entry point's other MK_ERR_ARG checks between them: made for another context, ...
static int genome_map_owned(const mk_ctx *c, const GenomeMap &m)
{
    if (m.owner == c) return MK_OK;
    set_error("the %s was made for another context", m.noun);
    return MK_ERR_ARG;
}

// ... made for other genomes
static int genome_map_fresh(const mk_ctx *c, const GenomeMap &m)
{
    if (m.index_id == c->index_id) return MK_OK;
    set_error("the %s was made before the index's genomes were selected or replaced: its %s name other genomes now", m.noun, m.names);
    return MK_ERR_STATE;
}

// ---- families: the list walk with a union-find forest as its sink (family.hip) ---------------------------------------------
// The walk pass over a set with the passing (query, genome) pairs joined by launch(chunk, the chunk's query ids on the device);
// a part of a mixed set runs with its queries' ids.  Everything is queued; nothing is waited for.
template <typename Launch>
static int qset_run_link_with(mk_ctx *c, mk_qset *qs, const uint32_t *query_ids, uint32_t min_score, double min_inter, Launch launch)
{
    return qset_leaves(c, qs, [&](mk_qset *leaf, const std::vector<uint32_t> *places) -> int {
        std::vector<uint32_t> ids;
        if (places) for (uint32_t q : *places) ids.push_back(query_ids[q]);
        mk_ctx::LinkScratch &ks = c->link;
        if (leaf->nq > ks.d_qid.cap) MK_HIP(hipStreamSynchronize(c->stream));    // (an earlier pass may still read the ids it was given)
        MK_TRY(ks.d_qid.grow(leaf->nq));
        // (from pageable memory: the host waits until the stream has reached the copy, so the array is free on return)
        MK_HIP(hipMemcpyAsync(ks.d_qid, places ? ids.data() : query_ids, (size_t)leaf->nq * 4, hipMemcpyHostToDevice, c->stream));
        return qset_walk(c, leaf, min_score, min_inter, [&](uint32_t q0, const ListArgs &a) { return launch(a, ks.d_qid + q0); });
    });
}

static int qset_run_link(mk_ctx *c, mk_qset *qs, const uint32_t *query_ids, uint32_t min_score, double min_inter, uint32_t *d_parent)
{
    return qset_run_link_with(c, qs, query_ids, min_score, min_inter, [&](const ListArgs &a, const uint32_t *d_qid) { return launch_link(c, LinkArgs{a, d_qid, d_parent}); });
}

// the levels of mk_qset_run_link_levels and mk_index_hierarchy: 1 .. MK_MAX_LEVELS of them, neither threshold falling
static int refuse_levels(const mk_level *levels, uint32_t n_levels)
{
    if (!levels) { set_error("null argument"); return MK_ERR_ARG; }
    if (n_levels < 1 || n_levels > MK_MAX_LEVELS) { set_error("%u levels: a hierarchy has 1 .. %d", n_levels, MK_MAX_LEVELS); return MK_ERR_ARG; }
    for (uint32_t l = 0; l < n_levels; ++l) {
        if (levels[l].min_intersection != levels[l].min_intersection) { set_error("level %u: min_intersection is not a number", l); return MK_ERR_ARG; }
        if (l && levels[l].min_score < levels[l - 1].min_score) {
            set_error("level %u: min_score %u is below level %u's %u (level 0 is the loosest)", l, levels[l].min_score, l - 1, levels[l - 1].min_score);
            return MK_ERR_ARG;
        }
        if (l && levels[l].min_intersection < levels[l - 1].min_intersection) {
            set_error("level %u: min_intersection %g is below level %u's %g (level 0 is the loosest)", l, levels[l].min_intersection, l - 1, levels[l - 1].min_intersection);
            return MK_ERR_ARG;
        }
    }
    return MK_OK;
}

extern "C" {

int mk_link_reset(mk_ctx *c, uint32_t *d_parent, uint32_t n_ids)
{
    if (!c || (n_ids && !d_parent)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return launch_link_reset(c, d_parent, n_ids);
}

int mk_qset_run_link(mk_ctx *c, mk_qset *qs, const uint32_t *query_ids, uint32_t min_score, double min_inter, uint32_t *d_parent,
                     uint32_t n_ids)
{
    if (!c || !qs || !d_parent || (qs->nq && !query_ids)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    for (uint32_t j = 0; j < qs->nq; ++j)
        if (query_ids[j] >= n_ids) { set_error("query %u stands for id %u, beyond the forest's %u ids", j, query_ids[j], n_ids); return MK_ERR_ARG; }
    MK_TRY(refuse_ids_beyond(c, n_ids, "forest"));
    MK_TRY(refuse_nan_lists(c, min_score));
    return qset_run_link(c, qs, query_ids, min_score, min_inter, d_parent);
}

int mk_link_merge(mk_ctx *c, uint32_t *d_parent, const uint32_t *d_other, uint32_t n_ids)
{
    if (!c || (n_ids && (!d_parent || !d_other))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return launch_link_merge(c, d_parent, d_other, n_ids);
}

int mk_link_labels(mk_ctx *c, const uint32_t *d_parent, uint32_t n_ids, uint32_t *labels)
{
    if (!c || (n_ids && (!d_parent || !labels))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (!n_ids) return MK_OK;
    mk_ctx::LinkScratch &ks = c->link;
    MK_TRY(ks.d_label.grow(n_ids));
    MK_TRY(launch_link_labels(c, d_parent, n_ids, ks.d_label));
    MK_HIP(hipMemcpyAsync(labels, ks.d_label, (size_t)n_ids * 4, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    return drain_timers(c);
}

int mk_index_families(mk_ctx *c, uint32_t min_score, double min_inter, uint32_t *labels)
{
    if (!c) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G, base = c->p.genome_id_base;
    if (!G) return MK_OK;
    if (!labels) { set_error("null argument"); return MK_ERR_ARG; }
    if ((uint64_t)base + G > 0xffffffffull) { set_error("genome ids beyond 32 bits"); return MK_ERR_ARG; }
    // the forest spans the ids the context reports, [0, base + G); the ids below base stay families of one
    const uint32_t n_ids = base + G;
    uint32_t *d_parent = nullptr;
    MK_TRY(dev_alloc(&d_parent, (uint64_t)n_ids));
    DevGuard<uint32_t> guard(d_parent);
    MK_TRY(launch_link_reset(c, d_parent, n_ids));
    MK_TRY(for_index_sets(c, index_set_ids(c), [&](mk_qset *qs, const uint32_t *ids, uint32_t, uint32_t) {
        return mk_qset_run_link(c, qs, ids, min_score, min_inter, d_parent, n_ids);
    }));
    std::vector<uint32_t> all(n_ids);
    MK_TRY(mk_link_labels(c, d_parent, n_ids, all.data()));
    std::copy(all.begin() + base, all.end(), labels);
    return MK_OK;
}

int mk_qset_run_link_levels(mk_ctx *c, mk_qset *qs, const uint32_t *query_ids, const mk_level *levels, uint32_t n_levels,
                            uint32_t *d_parents, uint32_t n_ids)
{
    if (!c || !qs || !d_parents || !levels || (qs->nq && !query_ids)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(refuse_levels(levels, n_levels));
    MK_TRY(use_device(c));
    for (uint32_t j = 0; j < qs->nq; ++j)
        if (query_ids[j] >= n_ids) { set_error("query %u stands for id %u, beyond the forests' %u ids", j, query_ids[j], n_ids); return MK_ERR_ARG; }
    MK_TRY(refuse_ids_beyond(c, n_ids, "forest"));
    MK_TRY(refuse_nan_lists(c, levels[0].min_score));
    LinkLevelsArgs k{};
    k.n_levels = n_levels; k.n_ids = n_ids;
    std::copy(levels, levels + n_levels, k.levels);
    return qset_run_link_with(c, qs, query_ids, levels[0].min_score, levels[0].min_intersection, [&](const ListArgs &a, const uint32_t *d_qid) {
        k.link = LinkArgs{a, d_qid, d_parents};
        return launch_link_levels(c, k);
    });
}

int mk_link_fold_levels(mk_ctx *c, uint32_t *d_parents, uint32_t n_ids, uint32_t n_levels)
{
    if (!c || (n_ids && !d_parents)) { set_error("null argument"); return MK_ERR_ARG; }
    if (n_levels < 1 || n_levels > MK_MAX_LEVELS) { set_error("%u levels: a hierarchy has 1 .. %d", n_levels, MK_MAX_LEVELS); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    for (uint32_t l = n_levels - 1; l-- > 0;)                      // strict to loose: forest l + 1 holds every stricter level already
        MK_TRY(launch_link_merge(c, d_parents + (size_t)l * n_ids, d_parents + (size_t)(l + 1) * n_ids, n_ids));
    return MK_OK;
}

int mk_index_hierarchy(mk_ctx *c, const mk_level *levels, uint32_t n_levels, uint32_t *labels)
{
    if (!c) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(refuse_levels(levels, n_levels));
    MK_TRY(use_device(c));
    const uint32_t G = c->G, base = c->p.genome_id_base;
    if (!G) return MK_OK;
    if (!labels) { set_error("null argument"); return MK_ERR_ARG; }
    if ((uint64_t)base + G > 0xffffffffull) { set_error("genome ids beyond 32 bits"); return MK_ERR_ARG; }
    // a forest per level over the ids the context reports, [0, base + G); the ids below base stay families of one
    const uint32_t n_ids = base + G;
    uint32_t *d_parents = nullptr;
    MK_TRY(dev_alloc(&d_parents, (uint64_t)n_levels * n_ids));
    DevGuard<uint32_t> guard(d_parents);
    for (uint32_t l = 0; l < n_levels; ++l) MK_TRY(launch_link_reset(c, d_parents + (size_t)l * n_ids, n_ids));
    MK_TRY(for_index_sets(c, index_set_ids(c), [&](mk_qset *qs, const uint32_t *ids, uint32_t, uint32_t) {
        return mk_qset_run_link_levels(c, qs, ids, levels, n_levels, d_parents, n_ids);
    }));
    MK_TRY(mk_link_fold_levels(c, d_parents, n_ids, n_levels));
    std::vector<uint32_t> all(n_ids);
    for (uint32_t l = 0; l < n_levels; ++l) {
        MK_TRY(mk_link_labels(c, d_parents + (size_t)l * n_ids, n_ids, all.data()));
        std::copy(all.begin() + base, all.end(), labels + (size_t)l * G);
    }
    return MK_OK;
}

}  // extern "C"

// ---- tallies: the list walk with four counters per genome as its sink (tally.hip) ------------------------------------------
// The walk pass over a set with every chunk's queries added to the counters of the context's own genomes, d_local[G] (a sum:
// whose query a count came from does not matter).  Everything is queued; nothing is waited for.
static int qset_run_tally(mk_ctx *c, mk_qset *qs, uint32_t min_score, double min_inter, mk_tally *d_local)
{
    return qset_leaves(c, qs, [&](mk_qset *leaf, const std::vector<uint32_t> *) {
        return qset_walk(c, leaf, min_score, min_inter, [&](uint32_t, const ListArgs &a) { return launch_tally(c, TallyArgs{a, d_local}); });
    });
}

extern "C" {

int mk_tally_reset(mk_ctx *c, mk_tally *d_tally, uint32_t n_ids) { return counters_reset(c, d_tally, n_ids); }

int mk_qset_run_tally(mk_ctx *c, mk_qset *qs, uint32_t min_score, double min_inter, mk_tally *d_tally, uint32_t n_ids)
{
    if (!c || !qs || !d_tally) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    MK_TRY(refuse_ids_beyond(c, n_ids, "tally"));
    MK_TRY(refuse_nan_lists(c, min_score));
    return qset_run_tally(c, qs, min_score, min_inter, d_tally + c->p.genome_id_base);
}

int mk_tally_read(mk_ctx *c, const mk_tally *d_tally, uint32_t n_ids, mk_tally *out) { return counters_read(c, d_tally, n_ids, out); }

int mk_query_tally(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t min_score, double min_inter,
                   mk_tally *tally)
{
    if (!c || (nq && (!seqs || !lens))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G;
    if (!G) return MK_OK;
    if (!tally) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(refuse_nan_lists(c, min_score));
    // counters of the context's own genomes only: the ids it reports play no part in a call that answers by local genome
    return query_counters(c, seqs, lens, nq, G, tally, [&](mk_qset *qs, uint32_t, mk_tally *d_local) { return qset_run_tally(c, qs, min_score, min_inter, d_local); });
}

}  // extern "C"

// ---- clade tallies: the list walk with five counters per clade of genomes as its sink (clade.hip) ---------------------------
// The map: the caller's numbers as a GenomeMap.
struct mk_clade_map {
    GenomeMap clade{"clade map", "entries"};
    uint32_t size = 0;             // 1 + the largest clade number, 0: every genome left out
};

// the host checks of a map; *size = 1 + the largest number
static int clade_map_check(const mk_ctx *c, const uint32_t *clade, uint32_t n, uint32_t *size)
{
    if (n != c->G) { set_error("the clade map has %u entries, the index holds %u genomes", n, c->G); return MK_ERR_ARG; }
    uint32_t last = 0;
    bool any = false;
    for (uint32_t j = 0; j < n; ++j) {
        if (clade[j] == MK_NO_CLADE) continue;
        if (any && clade[j] < last) {
            set_error("clade numbers must not decrease along the genome ids: genome %u has clade %u after clade %u (reorder with mk_index_select)", j, clade[j], last);
            return MK_ERR_ARG;
        }
        last = clade[j];
        any = true;
    }
    *size = any ? last + 1 : 0;
    return MK_OK;
}

static int clade_map_make(mk_ctx *c, const uint32_t *clade, uint32_t n, mk_clade_map **out)
{
    std::unique_ptr<mk_clade_map> m(new mk_clade_map);
    MK_TRY(clade_map_check(c, clade, n, &m->size));
    MK_TRY(genome_map_make(c, m->clade, clade, n));
    *out = m.release();
    return MK_OK;
}

// The walk pass over a set with every chunk's queries added to the clade counters and, where d_local is given, to the plain
// counters of the context's own genomes: both sinks on each chunk of the one scan.  Everything is queued.
static int qset_run_clade_tally(mk_ctx *c, mk_qset *qs, uint32_t min_score, double min_inter, const mk_clade_map *map, mk_clade_tally *d_ct,
                                mk_tally *d_local)
{
    const bool clades = map->size != 0;                            // (nothing to count: the plain tally alone)
    if (!clades && !d_local) return qset_checks_only(c, qs);
    return qset_leaves(c, qs, [&](mk_qset *leaf, const std::vector<uint32_t> *) {
        return qset_walk(c, leaf, min_score, min_inter, [&](uint32_t, const ListArgs &a) -> int {
            if (d_local) MK_TRY(launch_tally(c, TallyArgs{a, d_local}));
            if (clades) MK_TRY(launch_clade_tally(c, CladeArgs{a, map->clade.d_word, map->clade.padded, d_ct}));
            return MK_OK;
        });
    });
}

extern "C" {

int mk_clade_map_create(mk_ctx *c, const uint32_t *clade, uint32_t n_genomes, mk_clade_map **out)
{
    if (!c || !out || (n_genomes && !clade)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return clade_map_make(c, clade, n_genomes, out);
}

uint32_t mk_clade_map_size(const mk_clade_map *map) { return map ? map->size : 0; }

void mk_clade_map_free(mk_ctx *c, mk_clade_map *map)
{
    if (!map) return;
    genome_map_wait(c, map->clade);
    delete map;
}

int mk_clade_tally_reset(mk_ctx *c, mk_clade_tally *d_ct, uint32_t n_clades) { return counters_reset(c, d_ct, n_clades); }

int mk_qset_run_clade_tally(mk_ctx *c, mk_qset *qs, uint32_t min_score, double min_inter, const mk_clade_map *map, mk_clade_tally *d_ct,
                            uint32_t n_clades, mk_tally *d_tally, uint32_t n_ids)
{
    if (!c || !qs || !map || !d_ct) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    MK_TRY(genome_map_owned(c, map->clade));
    if (n_clades < map->size) { set_error("the clade map numbers clades up to %u, beyond the counters' %u clades", map->size - 1, n_clades); return MK_ERR_ARG; }
    if (d_tally) MK_TRY(refuse_ids_beyond(c, n_ids, "tally"));
    MK_TRY(refuse_nan_lists(c, min_score));
    MK_TRY(genome_map_fresh(c, map->clade));
    return qset_run_clade_tally(c, qs, min_score, min_inter, map, d_ct, d_tally ? d_tally + c->p.genome_id_base : nullptr);
}

int mk_clade_tally_read(mk_ctx *c, const mk_clade_tally *d_ct, uint32_t n_clades, mk_clade_tally *out) { return counters_read(c, d_ct, n_clades, out); }

int mk_query_clade_tally(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t min_score, double min_inter,
                         const uint32_t *clade, uint32_t n_clades, mk_clade_tally *out)
{
    if (!c || (nq && (!seqs || !lens))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G;
    if (!G) return MK_OK;
    if (!clade || (n_clades && !out)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(refuse_nan_lists(c, min_score));
    uint32_t size = 0;
    MK_TRY(clade_map_check(c, clade, G, &size));                   // (before anything is uploaded)
    if (n_clades < size) { set_error("the clade map numbers clades up to %u, beyond the counters' %u clades", size - 1, n_clades); return MK_ERR_ARG; }
    mk_clade_map *made = nullptr;
    MK_TRY(clade_map_make(c, clade, G, &made));
    std::unique_ptr<mk_clade_map> map(made);                       // (goes on return: the read at the end has waited)
    return query_counters(c, seqs, lens, nq, n_clades, out, [&](mk_qset *qs, uint32_t, mk_clade_tally *d_ct) {
        return qset_run_clade_tally(c, qs, min_score, min_inter, map.get(), d_ct, nullptr);
    });
}

}  // extern "C"

// ---- lca: the list walk with three counters per node of a taxonomy as its sink (lca.hip) ------------------------------------
// The taxonomy: what one stack pass over the caller's intervals derives -- parent, leaf, the largest depth -- with leaf as a
// GenomeMap.
struct mk_taxonomy {
    GenomeMap leaf{"taxonomy", "intervals"};
    uint32_t n_nodes = 0;
    uint32_t depth = 0;            // the largest number of ancestors of any node
    uint32_t *d_parent = nullptr, *d_hi = nullptr, *d_lo = nullptr;
    uint32_t *d_live = nullptr;    // a bit per genome of leaf.padded: it has a leaf (mk_taxonomy_markers)
    std::vector<uint32_t> parent;  // host copy (mk_taxonomy_parents)
    std::vector<uint32_t> lo, hi;  // host copies: the node pass's work list (mk_taxonomy_cover)
    ~mk_taxonomy()
    {
        if (d_parent) (void)hipFree(d_parent);
        if (d_hi) (void)hipFree(d_hi);
        if (d_lo) (void)hipFree(d_lo);
        if (d_live) (void)hipFree(d_live);
    }
};

// The host checks and the derivation, one pass with a stack of the open nodes: parent[n_nodes], leaf[n_genomes], *depth
static int taxonomy_derive(const uint32_t *lo, const uint32_t *hi, uint32_t n_nodes, uint32_t n_genomes, std::vector<uint32_t> &parent,
                           std::vector<uint32_t> &leaf, uint32_t *depth)
{
    parent.assign(n_nodes, MK_NO_NODE);
    leaf.assign(n_genomes, MK_NO_NODE);
    *depth = 0;
    std::vector<uint32_t> open;                                    // the nodes that contain the current position, outermost first
    uint32_t at = 0;                                               // genomes below `at` have their leaf
    auto fill_to = [&](uint32_t end) {                             // the genomes [at, end) lie in the innermost open node, or in none
        const uint32_t v = open.empty() ? MK_NO_NODE : open.back();
        for (; at < end; ++at) leaf[at] = v;
    };
    for (uint32_t v = 0; v < n_nodes; ++v) {
        if (lo[v] >= hi[v]) { set_error("node %u is the empty interval [%u, %u)", v, lo[v], hi[v]); return MK_ERR_ARG; }
        if (hi[v] > n_genomes) { set_error("node %u ends at genome %u, beyond the index's %u genomes", v, hi[v], n_genomes); return MK_ERR_ARG; }
        if (v && lo[v] == lo[v - 1] && hi[v] == hi[v - 1]) { set_error("node %u is a duplicate of node %u, [%u, %u)", v, v - 1, lo[v], hi[v]); return MK_ERR_ARG; }
        if (v && (lo[v] < lo[v - 1] || (lo[v] == lo[v - 1] && hi[v] > hi[v - 1]))) {
            set_error("node %u, [%u, %u), comes after node %u, [%u, %u): the nodes are not in preorder (a parent before its children, by ascending first id)",
                      v, lo[v], hi[v], v - 1, lo[v - 1], hi[v - 1]);
            return MK_ERR_ARG;
        }
        while (!open.empty() && hi[open.back()] <= lo[v]) { fill_to(hi[open.back()]); open.pop_back(); }
        if (!open.empty() && hi[v] > hi[open.back()]) {
            set_error("node %u, [%u, %u), overlaps node %u, [%u, %u), without lying inside it", v, lo[v], hi[v], open.back(), lo[open.back()], hi[open.back()]);
            return MK_ERR_ARG;
        }
        fill_to(lo[v]);
        if (!open.empty()) parent[v] = open.back();
        *depth = std::max<uint32_t>(*depth, (uint32_t)open.size());
        open.push_back(v);
    }
    while (!open.empty()) { fill_to(hi[open.back()]); open.pop_back(); }
    return MK_OK;
}

static int taxonomy_make(mk_ctx *c, const uint32_t *lo, const uint32_t *hi, uint32_t n_nodes, uint32_t n, mk_taxonomy **out)
{
    if (n != c->G) { set_error("the taxonomy is over %u genomes, the index holds %u", n, c->G); return MK_ERR_ARG; }
    std::unique_ptr<mk_taxonomy> t(new mk_taxonomy);
    std::vector<uint32_t> leaf, live;
    MK_TRY(taxonomy_derive(lo, hi, n_nodes, n, t->parent, leaf, &t->depth));
    t->n_nodes = n_nodes;
    t->lo.assign(lo, lo + n_nodes);
    t->hi.assign(hi, hi + n_nodes);
    if (n && n_nodes) {                                            // (no genomes or no nodes: no pass walks it, nothing goes up)
        MK_TRY(dev_alloc(&t->d_parent, (uint64_t)n_nodes));
        MK_TRY(dev_alloc(&t->d_hi, (uint64_t)n_nodes));
        MK_TRY(dev_alloc(&t->d_lo, (uint64_t)n_nodes));
        MK_HIP(hipMemcpyAsync(t->d_parent, t->parent.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, c->stream));
        MK_HIP(hipMemcpyAsync(t->d_hi, hi, (size_t)n_nodes * 4, hipMemcpyHostToDevice, c->stream));
        MK_HIP(hipMemcpyAsync(t->d_lo, lo, (size_t)n_nodes * 4, hipMemcpyHostToDevice, c->stream));
        const uint64_t padded = ((uint64_t)n + kTileBytes - 1) / kTileBytes * kTileBytes;             // (the leaf map's)
        live.assign(padded / 32, 0u);
        for (uint32_t g = 0; g < n; ++g) if (leaf[g] != MK_NO_NODE) live[g >> 5] |= 1u << (g & 31u);
        MK_TRY(dev_alloc(&t->d_live, padded / 32));
        MK_HIP(hipMemcpyAsync(t->d_live, live.data(), (size_t)(padded / 32) * 4, hipMemcpyHostToDevice, c->stream));
    }
    MK_TRY(genome_map_make(c, t->leaf, leaf.data(), n, n_nodes != 0));     // (its wait is the one wait for all five copies)
    *out = t.release();
    return MK_OK;
}

// The walk pass over a set with every chunk's queries added to their nodes' counters and, where d_node is given, every query's
// node written at its place in the set: a part of a mixed set brings its queries' places, which the set keeps on the device.
// Everything is queued.
static int qset_run_lca(mk_ctx *c, mk_qset *qs, uint32_t min_score, double min_inter, uint32_t margin, const mk_taxonomy *tax, mk_lca_tally *d_lt,
                        uint32_t *d_node)
{
    if (d_node && qs->nq) MK_HIP(hipMemsetAsync(d_node, 0xff, (size_t)qs->nq * 4, c->stream));   // MK_NO_NODE: queries that no launch reaches
    if (!tax->n_nodes) return qset_checks_only(c, qs);
    return qset_leaves(c, qs, [&](mk_qset *leaf, const std::vector<uint32_t> *places) {
        const uint32_t *d_place = !places ? nullptr : qs->d_part_q[places == &qs->part_q[1] ? 1 : 0];
        return qset_walk(c, leaf, min_score, min_inter, [&](uint32_t q0, const ListArgs &a) {
            return launch_lca(c, LcaArgs{a, tax->leaf.d_word, tax->leaf.padded, tax->d_parent, tax->d_hi, tax->n_nodes, tax->depth, margin, d_lt, d_node, d_place, q0});
        });
    });
}

extern "C" {

int mk_taxonomy_create(mk_ctx *c, const uint32_t *lo, const uint32_t *hi, uint32_t n_nodes, uint32_t n_genomes, mk_taxonomy **out)
{
    if (!c || !out || (n_nodes && (!lo || !hi))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return taxonomy_make(c, lo, hi, n_nodes, n_genomes, out);
}

uint32_t mk_taxonomy_nodes(const mk_taxonomy *tax) { return tax ? tax->n_nodes : 0; }

int mk_taxonomy_parents(const mk_taxonomy *tax, uint32_t *parent_out)
{
    if (!tax || (tax->n_nodes && !parent_out)) { set_error("null argument"); return MK_ERR_ARG; }
    std::copy(tax->parent.begin(), tax->parent.end(), parent_out);
    return MK_OK;
}

void mk_taxonomy_free(mk_ctx *c, mk_taxonomy *tax)
{
    if (!tax) return;
    genome_map_wait(c, tax->leaf);
    delete tax;
}

int mk_lca_tally_reset(mk_ctx *c, mk_lca_tally *d_lt, uint32_t n_slots) { return counters_reset(c, d_lt, n_slots); }

int mk_qset_run_lca(mk_ctx *c, mk_qset *qs, uint32_t min_score, double min_inter, uint32_t margin, const mk_taxonomy *tax, mk_lca_tally *d_lt,
                    uint32_t n_slots, uint32_t *d_node)
{
    if (!c || !qs || !tax || !d_lt) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    MK_TRY(genome_map_owned(c, tax->leaf));
    if ((uint64_t)n_slots < (uint64_t)tax->n_nodes + 1) { set_error("the taxonomy has %u nodes and the slot above them, beyond the counters' %u slots", tax->n_nodes, n_slots); return MK_ERR_ARG; }
    if (margin > 100) { set_error("the margin is a percentage, 0 .. 100: %u", margin); return MK_ERR_ARG; }
    MK_TRY(refuse_nan_lists(c, min_score));
    MK_TRY(genome_map_fresh(c, tax->leaf));
    return qset_run_lca(c, qs, min_score, min_inter, margin, tax, d_lt, d_node);
}

int mk_lca_tally_read(mk_ctx *c, const mk_lca_tally *d_lt, uint32_t n_slots, mk_lca_tally *out) { return counters_read(c, d_lt, n_slots, out); }

int mk_query_lca(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t min_score, double min_inter, uint32_t margin,
                 const uint32_t *lo, const uint32_t *hi, uint32_t n_nodes, mk_lca_tally *out_tally, uint32_t *out_node)
{
    if (!c || (nq && (!seqs || !lens))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G;
    if (!G) return MK_OK;
    if (!out_tally || (n_nodes && (!lo || !hi))) { set_error("null argument"); return MK_ERR_ARG; }
    if (margin > 100) { set_error("the margin is a percentage, 0 .. 100: %u", margin); return MK_ERR_ARG; }
    MK_TRY(refuse_nan_lists(c, min_score));
    mk_taxonomy *made = nullptr;
    MK_TRY(taxonomy_make(c, lo, hi, n_nodes, G, &made));
    std::unique_ptr<mk_taxonomy> tax(made);                        // (goes on return: the read at the end has waited)
    uint32_t *d_node = nullptr;
    if (out_node && nq) MK_TRY(dev_alloc(&d_node, (uint64_t)nq));
    DevGuard<uint32_t> node_guard(d_node);
    // (a slice's nodes go behind those of the slices before; their copy is queued before the counters' read, which waits)
    return query_counters(c, seqs, lens, nq, n_nodes + 1, out_tally, [&](mk_qset *qs, uint32_t q0, mk_lca_tally *d_lt) {
        return qset_run_lca(c, qs, min_score, min_inter, margin, tax.get(), d_lt, d_node ? d_node + q0 : nullptr);
    }, [&]() -> int {
        if (d_node) MK_HIP(hipMemcpyAsync(out_node, d_node, (size_t)nq * 4, hipMemcpyDeviceToHost, c->stream));
        return MK_OK;
    });
}

}  // extern "C"

// ---- share: the list walk with a pool of per-read genome lists as its sink, and the EM rounds over the pool (share.hip) ------
// The pool: unique[G] and shared[G], the shared reads' ids and offsets, the rounds' two buffers and the collect pass's
// per-chunk scratch on the device; on the host what the pool holds -- the collect pass reads a chunk's totals back to grow
// it, so the host always knows -- and what the ids meant when it was made.
struct mk_sharepool {
    mk_ctx *owner = nullptr;
    uint32_t G = 0;
    uint64_t index_id = 0;         // the context's index_id when it was made -- another value: the ids name other genomes
    bool broken = false;           // a growth failed in the middle of a pass: MK_ERR_STATE until mk_share_reset
    uint64_t queries = 0, settled = 0, reads = 0, entries = 0;
    DevArray<uint64_t> d_counts;   // [unique: G][shared: G][settled of the chunk in flight, delta, starved]
    DevArray<uint64_t> d_A;        // [2][G]
    DevArray<uint32_t> d_ids;      // entries
    DevArray<uint64_t> d_off;      // reads + 1, d_off[0] = 0
    DevArray<uint32_t> d_count;    // the chunk in flight: |K| of its shared queries,
    DevArray<uint64_t> d_scan;     // ... [2][n + 1] the scans: ids, lists,
    DevArray<double> d_least;      // ... the margin's right-hand sides
    uint64_t *unique() const { return d_counts; }
    uint64_t *shared() const { return d_counts + G; }
    uint64_t *words() const { return d_counts + 2 * (uint64_t)G; }
};

// the refusals of a pool: made for another context (MK_ERR_ARG), for other genomes or left half-filled (MK_ERR_STATE)
static int share_usable(const mk_ctx *c, const mk_sharepool *pool)
{
    if (pool->owner != c) { set_error("the share pool was made for another context"); return MK_ERR_ARG; }
    if (pool->index_id != c->index_id || pool->G != c->G) {
        set_error("the share pool was made for %u genomes before the index's genomes were selected, replaced or added to: its ids name other genomes now", pool->G);
        return MK_ERR_STATE;
    }
    if (pool->broken) { set_error("the share pool could not grow in the middle of a pass: mk_share_reset empties it"); return MK_ERR_STATE; }
    return MK_OK;
}

// room for `need` elements with the first `used` kept (the stream is waited for: queued work may read the old array)
template <typename T>
static int share_grow(mk_ctx *c, DevArray<T> &a, uint64_t used, uint64_t need)
{
    if (need <= a.cap) return MK_OK;
    DevArray<T> bigger;
    const uint64_t room = need + need / 2;
    if (hipMalloc((void **)&bigger.p, room * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        bigger.p = nullptr;
        (void)gz_release_idle_blocks();
        if (hipMalloc((void **)&bigger.p, room * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            bigger.p = nullptr;
            set_error("no room for a share pool of %llu bytes", (unsigned long long)(room * sizeof(T)));
            return MK_ERR_NOMEM;
        }
    }
    bigger.cap = room;
    if (used) MK_HIP(hipMemcpyAsync(bigger.p, a.p, (size_t)used * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    a = std::move(bigger);                                         // (the old array goes with `bigger`)
    return MK_OK;
}

static int share_clear(mk_ctx *c, mk_sharepool *pool)
{
    MK_HIP(hipMemsetAsync(pool->d_counts, 0, (2 * (size_t)pool->G + 3) * 8, c->stream));
    MK_HIP(hipMemsetAsync(pool->d_off, 0, 8, c->stream));
    pool->queries = pool->settled = pool->reads = pool->entries = 0;
    pool->broken = false;
    return MK_OK;
}

// The walk pass over a set with every chunk's queries sorted into unassigned, settled and shared: count, scan, ONE read of
// the chunk's totals (which waits), growth, write.
static int qset_run_share(mk_ctx *c, mk_qset *qs, uint32_t min_score, double min_inter, uint32_t margin, mk_sharepool *pool)
{
    if (!c->G) { MK_TRY(qset_checks_only(c, qs)); pool->queries += qs->nq; return MK_OK; }
    return qset_leaves(c, qs, [&](mk_qset *leaf, const std::vector<uint32_t> *) {
        return qset_walk(c, leaf, min_score, min_inter, [&](uint32_t, const ListArgs &chunk) -> int {
            const uint64_t n = chunk.q_n;
            if (n > pool->d_count.cap) {
                MK_HIP(hipStreamSynchronize(c->stream));             // (the write pass of the chunk before may still read them)
                MK_TRY(pool->d_count.grow(n));
                MK_TRY(pool->d_scan.grow(2 * (n + 1)));
                MK_TRY(pool->d_least.grow(n));
            }
            uint64_t *d_id_off = pool->d_scan, *d_read_off = pool->d_scan + (n + 1), *d_settled = pool->words();
            ShareArgs k{chunk, margin, pool->d_least, d_read_off, pool->unique(), pool->shared(), d_settled, nullptr, nullptr, pool->entries, pool->reads};
            k.list.count = pool->d_count; k.list.rec_off = d_id_off;
            MK_HIP(hipMemsetAsync(d_settled, 0, 8, c->stream));
            MK_TRY(launch_share_count(c, k));
            MK_TRY(launch_list_scan(c, pool->d_count, (uint32_t)n, 1, d_id_off, d_read_off));
            uint64_t got[3] = {0, 0, 0};                            // the chunk's ids, lists, settled queries
            MK_HIP(hipMemcpyAsync(&got[0], d_id_off + n, 8, hipMemcpyDeviceToHost, c->stream));
            MK_HIP(hipMemcpyAsync(&got[1], d_read_off + n, 8, hipMemcpyDeviceToHost, c->stream));
            MK_HIP(hipMemcpyAsync(&got[2], d_settled, 8, hipMemcpyDeviceToHost, c->stream));
            MK_HIP(hipStreamSynchronize(c->stream));
            pool->queries += n;
            pool->settled += got[2];
            if (!got[1]) return MK_OK;
            pool->broken = true;                                     // (until the chunk's lists are in)
            MK_TRY(share_grow(c, pool->d_ids, pool->entries, pool->entries + got[0]));
            MK_TRY(share_grow(c, pool->d_off, pool->reads + 1, pool->reads + got[1] + 1));
            k.ids = pool->d_ids; k.off = pool->d_off;
            MK_TRY(launch_share_write(c, k));
            pool->entries += got[0];
            pool->reads += got[1];
            pool->broken = false;
            return MK_OK;
        });
    });
}

static uint32_t bit_length(uint64_t v) { uint32_t n = 0; for (; v; v >>= 1) ++n; return n; }

extern "C" {

int mk_share_create(mk_ctx *c, mk_sharepool **out)
{
    if (!c || !out) { set_error("null argument"); return MK_ERR_ARG; }
    *out = nullptr;
    MK_TRY(use_device(c));
    std::unique_ptr<mk_sharepool> pool(new mk_sharepool);
    pool->owner = c; pool->G = c->G; pool->index_id = c->index_id;
    MK_TRY(pool->d_counts.alloc(2 * (uint64_t)c->G + 3));
    MK_TRY(pool->d_A.alloc(2 * (uint64_t)std::max<uint32_t>(c->G, 1)));
    MK_TRY(pool->d_ids.alloc(4096));
    MK_TRY(pool->d_off.alloc(1024));
    MK_TRY(share_clear(c, pool.get()));
    *out = pool.release();
    return MK_OK;
}

void mk_share_free(mk_ctx *c, mk_sharepool *pool)
{
    if (!pool) return;
    mk_ctx *owner = c ? c : pool->owner;                           // (a queued pass or round may still read the pool)
    if (owner && use_device(owner, false) == MK_OK) (void)hipStreamSynchronize(owner->stream);
    delete pool;
}

int mk_share_reset(mk_ctx *c, mk_sharepool *pool)
{
    if (!c || !pool) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (pool->owner != c) { set_error("the share pool was made for another context"); return MK_ERR_ARG; }
    return share_clear(c, pool);
}

int mk_qset_run_share(mk_ctx *c, mk_qset *qs, uint32_t min_score, double min_inter, uint32_t margin, mk_sharepool *pool)
{
    if (!c || !qs || !pool) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (pool->owner != c) { set_error("the share pool was made for another context"); return MK_ERR_ARG; }
    if (margin > 100) { set_error("the margin is a percentage, 0 .. 100: %u", margin); return MK_ERR_ARG; }
    MK_TRY(refuse_nan_lists(c, min_score));
    MK_TRY(share_usable(c, pool));
    MK_TRY(qset_run_share(c, qs, min_score, min_inter, margin, pool));
    return drain_timers(c);
}

int mk_share_add_lists(mk_ctx *c, mk_sharepool *pool, const uint64_t *offsets, const uint32_t *ids, uint32_t n_lists)
{
    if (!c || !pool || !offsets || (n_lists && offsets[n_lists] && !ids)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    MK_TRY(share_usable(c, pool));
    std::vector<uint32_t> alone, several;                           // the settled lists' ids; the shared lists' ids, one behind the other
    std::vector<uint64_t> ends;                                     // the shared lists' ends in the pool
    for (uint32_t i = 0; i < n_lists; ++i) {
        if (offsets[i + 1] < offsets[i]) { set_error("list %u ends at %llu, before it begins", i, (unsigned long long)offsets[i + 1]); return MK_ERR_ARG; }
        const uint64_t len = offsets[i + 1] - offsets[i];
        const uint32_t *l = ids + offsets[i];
        for (uint64_t j = 0; j < len; ++j) {
            if (l[j] >= pool->G) { set_error("list %u names genome %u, beyond the pool's %u genomes", i, l[j], pool->G); return MK_ERR_ARG; }
            if (j && l[j] <= l[j - 1]) { set_error("list %u is not strictly ascending: %u after %u", i, l[j], l[j - 1]); return MK_ERR_ARG; }
        }
        if (len == 1) alone.push_back(l[0]);
        if (len < 2) continue;
        several.insert(several.end(), l, l + len);
        ends.push_back(pool->entries + several.size());
    }
    // (the settled ids go up behind the shared ones, as scratch: the next lists overwrite them)
    pool->broken = true;
    MK_TRY(share_grow(c, pool->d_ids, pool->entries, pool->entries + several.size() + alone.size()));
    MK_TRY(share_grow(c, pool->d_off, pool->reads + 1, pool->reads + ends.size() + 1));
    uint32_t *d_new = pool->d_ids + pool->entries, *d_alone = d_new + several.size();
    // (from pageable memory; the wait at the end is before the vectors go)
    if (!several.empty()) MK_HIP(hipMemcpyAsync(d_new, several.data(), several.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!alone.empty()) MK_HIP(hipMemcpyAsync(d_alone, alone.data(), alone.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!ends.empty()) MK_HIP(hipMemcpyAsync(pool->d_off + pool->reads + 1, ends.data(), ends.size() * 8, hipMemcpyHostToDevice, c->stream));
    {
        ScopedTimer t(c, 2);
        MK_TRY(launch_share_bump(c, d_new, several.size(), pool->shared()));
        MK_TRY(launch_share_bump(c, d_alone, alone.size(), pool->unique()));
    }
    MK_HIP(hipStreamSynchronize(c->stream));
    pool->queries += n_lists;
    pool->settled += alone.size();
    pool->reads += ends.size();
    pool->entries += several.size();
    pool->broken = false;
    return drain_timers(c);
}

int mk_share_info_read(mk_ctx *c, const mk_sharepool *pool, mk_share_info *out)
{
    if (!c || !pool || !out) { set_error("null argument"); return MK_ERR_ARG; }
    if (pool->owner != c) { set_error("the share pool was made for another context"); return MK_ERR_ARG; }
    *out = mk_share_info{pool->queries, pool->settled + pool->reads, pool->reads, pool->entries};
    return MK_OK;
}

int mk_share_export(mk_ctx *c, const mk_sharepool *pool, uint64_t *unique, uint64_t *shared, uint64_t *offsets, uint32_t *ids)
{
    if (!c || !pool) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (pool->owner != c) { set_error("the share pool was made for another context"); return MK_ERR_ARG; }
    if (pool->broken) { set_error("the share pool could not grow in the middle of a pass: mk_share_reset empties it"); return MK_ERR_STATE; }
    const size_t G = pool->G;
    if (unique && G) MK_HIP(hipMemcpyAsync(unique, pool->unique(), G * 8, hipMemcpyDeviceToHost, c->stream));
    if (shared && G) MK_HIP(hipMemcpyAsync(shared, pool->shared(), G * 8, hipMemcpyDeviceToHost, c->stream));
    if (offsets) MK_HIP(hipMemcpyAsync(offsets, pool->d_off, (size_t)(pool->reads + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (ids && pool->entries) MK_HIP(hipMemcpyAsync(ids, pool->d_ids, (size_t)pool->entries * 4, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    return drain_timers(c);
}

int mk_share_rounds(mk_ctx *c, mk_sharepool *pool, uint32_t rounds, uint32_t shift, uint64_t *abundance, mk_share_result *res)
{
    if (!c || !pool || !res || (pool->G && !abundance)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (pool->owner != c) { set_error("the share pool was made for another context"); return MK_ERR_ARG; }
    if (!rounds) { set_error("the rounds are 1 or more"); return MK_ERR_ARG; }
    MK_TRY(share_usable(c, pool));
    const uint64_t N = pool->settled + pool->reads;
    if (N >> 32) { set_error("%llu assigned queries: the weights are 32-bit fractions of fewer than 2^32 reads", (unsigned long long)N); return MK_ERR_UNSUPPORTED; }
    const uint32_t least = bit_length(N);
    if (shift == MK_SHARE_AUTO_SHIFT) shift = least;
    if (shift < least || shift > 32) { set_error("the shift is %u .. 32 for %llu assigned queries: %u", least, (unsigned long long)N, shift); return MK_ERR_ARG; }
    uint32_t team = 0;
    MK_TRY(share_team(&team));
    const uint32_t G = pool->G;
    uint64_t *d_delta = pool->words() + 1, *d_starved = pool->words() + 2;
    uint64_t got[2] = {0, 0};
    if (G) {
        ScopedTimer t(c, 2);
        MK_HIP(hipMemsetAsync(d_delta, 0, 16, c->stream));
        for (uint32_t r = 1; r <= rounds; ++r) {
            uint64_t *next = pool->d_A + (uint64_t)(r & 1u) * G, *prev = pool->d_A + (uint64_t)(~r & 1u) * G;
            MK_TRY(launch_share_seed(c, pool->unique(), G, next));
            MK_TRY(launch_share_round(c, RoundArgs{pool->d_ids, pool->d_off, pool->reads, r == 1 ? nullptr : prev, next, shift, r == rounds ? d_starved : nullptr}, team));
        }
        const uint64_t *last = pool->d_A + (uint64_t)(rounds & 1u) * G, *before = pool->d_A + (uint64_t)(~rounds & 1u) * G;
        MK_TRY(launch_share_delta(c, last, rounds == 1 ? nullptr : before, G, d_delta));
        MK_HIP(hipMemcpyAsync(abundance, last, (size_t)G * 8, hipMemcpyDeviceToHost, c->stream));
        MK_HIP(hipMemcpyAsync(got, d_delta, 16, hipMemcpyDeviceToHost, c->stream));
    }
    MK_HIP(hipStreamSynchronize(c->stream));
    *res = mk_share_result{got[0], got[1], rounds, shift};
    return drain_timers(c);
}

int mk_query_abundance(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t min_score, double min_inter, uint32_t margin,
                       uint32_t rounds, uint64_t *abundance, uint64_t *unique, uint64_t *shared, mk_share_info *info, mk_share_result *res)
{
    if (!c || (nq && (!seqs || !lens)) || !res || (c->G && !abundance)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (margin > 100) { set_error("the margin is a percentage, 0 .. 100: %u", margin); return MK_ERR_ARG; }
    if (!rounds) { set_error("the rounds are 1 or more"); return MK_ERR_ARG; }
    MK_TRY(refuse_nan_lists(c, min_score));
    mk_sharepool *made = nullptr;
    MK_TRY(mk_share_create(c, &made));
    std::unique_ptr<mk_sharepool> pool(made);                      // (goes on return: every step below has waited)
    MK_TRY(for_uploaded_slices(c, seqs, lens, nq, [&](mk_qset *qs, uint32_t, uint32_t) { return qset_run_share(c, qs, min_score, min_inter, margin, pool.get()); }));
    MK_TRY(mk_share_rounds(c, pool.get(), rounds, MK_SHARE_AUTO_SHIFT, abundance, res));
    if (unique || shared) MK_TRY(mk_share_export(c, pool.get(), unique, shared, nullptr, nullptr));
    if (info) MK_TRY(mk_share_info_read(c, pool.get(), info));
    return MK_OK;
}

}  // extern "C"

// ---- cover: the gated sketch of a set OR-ed into a table of (partition, value) bits, and one pass over the matrix that
// counts per genome the stored fingerprints the table holds (cover.hip).  No scan, no chunks: a set needs its sketch only.
// A set that a scan has prepared against this index keeps what it has; any other is sketched without the slab tables
// (qset_sketch_only) and stays "not prepared", so that a later scan of the same set makes them.  The depth's table (below)
// takes a set the same way: `launch` queues the marks of a sketched set that is not a shell over parts.
template <class Launch>
static int qset_mark(mk_ctx *c, mk_qset *qs, const Launch &launch)
{
    if (qs->part[0]) {
        // a mixed set: part by part (an OR, a sum: whose query a mark came from does not matter)
        for (int i = 0; i < 2; ++i) MK_TRY(qset_mark(c, qs->part[i], launch));
        return MK_OK;
    }
    if (!qs->nq) return MK_OK;
    const bool ready = qs->sketched && qs->gen == c->gen;
    if (!c->G && !qs->from_index) return MK_OK;
    if (!ready) {
        MK_TRY(qset_sketch_only(c, qs));                          // (a stale set made from the index: MK_ERR_STATE, before any launch)
        qs->sketched = false;
    }
    if (!c->G) return MK_OK;
    ScopedTimer t(c, 2);
    return launch(qs);
}

// a (partition, value) table of a call's own: when memory is short, the inflater's idle blocks go first
template <class T>
static int table_alloc(T **d_table, uint64_t bytes)
{
    *d_table = nullptr;
    if (hipMalloc((void **)d_table, bytes) == hipSuccess) return MK_OK;
    (void)hipGetLastError();
    *d_table = nullptr;
    (void)gz_release_idle_blocks();
    MK_HIP(hipMalloc((void **)d_table, bytes));                   // (out of memory: MK_ERR_NOMEM)
    return MK_OK;
}

// fresh tables of uploaded sequences (either may be null): reset, then per slice mk_qset_run_cover's pass and mk_qset_run_depth's
// (in slices: an OR and min(255, count) leave no trace of the slicing)
static int mark_uploaded(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t *d_seen, uint8_t *d_mult)
{
    if (d_seen) MK_TRY(launch_cover_reset(c, d_seen));
    if (d_mult) MK_TRY(launch_depth_reset(c, d_mult));
    return for_uploaded_slices(c, seqs, lens, nq, [&](mk_qset *qs, uint32_t, uint32_t) -> int {
        if (d_seen) MK_TRY(qset_mark(c, qs, [&](const mk_qset *leaf) { return launch_cover_mark(c, leaf, d_seen); }));
        if (d_mult) MK_TRY(qset_mark(c, qs, [&](const mk_qset *leaf) { return launch_depth_mark(c, leaf, d_mult); }));
        return MK_OK;
    });
}

extern "C" {

uint64_t mk_cover_bytes(const mk_ctx *c) { return c ? cover_table_bytes(c) : 0; }

int mk_cover_reset(mk_ctx *c, uint32_t *d_seen)
{
    if (!c || !d_seen) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return launch_cover_reset(c, d_seen);
}

int mk_qset_run_cover(mk_ctx *c, mk_qset *qs, uint32_t *d_seen)
{
    if (!c || !qs || !d_seen) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return qset_mark(c, qs, [&](const mk_qset *leaf) { return launch_cover_mark(c, leaf, d_seen); });
}

int mk_cover_count(mk_ctx *c, const uint32_t *d_seen, uint32_t *covered, uint64_t *cells)
{
    if (!c || !d_seen) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G;
    if (G && !covered) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(need_raw_cold(c));                                     // (the rule the exports follow: packed cold rows are unpacked first)
    // [cells: 8 bytes][covered: G words], zeroed, added to by the kernels, copied out
    uint32_t *d_out = nullptr;
    MK_TRY(dev_alloc(&d_out, (uint64_t)G + 2));
    DevGuard<uint32_t> guard(d_out);
    MK_HIP(hipMemsetAsync(d_out, 0, ((size_t)G + 2) * 4, c->stream));
    {
        ScopedTimer t(c, 2);
        MK_TRY(launch_cover_count(c, d_seen, G ? d_out + 2 : nullptr, cells ? reinterpret_cast<unsigned long long *>(d_out) : nullptr));
    }
    if (G) MK_HIP(hipMemcpyAsync(covered, d_out + 2, (size_t)G * 4, hipMemcpyDeviceToHost, c->stream));
    if (cells) MK_HIP(hipMemcpyAsync(cells, d_out, 8, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    return drain_timers(c);
}

int mk_query_cover(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t *covered, uint64_t *cells)
{
    if (!c || (nq && (!seqs || !lens))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (!c->G) { if (cells) *cells = 0; return MK_OK; }
    if (!covered) { set_error("null argument"); return MK_ERR_ARG; }
    uint32_t *d_seen = nullptr;
    MK_TRY(table_alloc(&d_seen, cover_table_bytes(c)));
    DevGuard<uint32_t> guard(d_seen);
    MK_TRY(mark_uploaded(c, seqs, lens, nq, d_seen, nullptr));
    return mk_cover_count(c, d_seen, covered, cells);                           // (waits: the table goes when this returns)
}

int mk_cover_assign(mk_ctx *c, const uint32_t *d_seen, const uint32_t *order, uint32_t *won, uint64_t *claimed)
{
    if (!c || !d_seen) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G;
    if (!G) { if (claimed) *claimed = 0; return MK_OK; }
    if (!order || !won) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(cover_win_values(c, nullptr));                         // (MIEKKI_WIN_VALUES: refused here, before anything is queued)
    // [rank: G][order: G][won: G]: the order and its inverse go up, 12 bytes per genome with the counts that come back
    std::vector<uint32_t> h((size_t)G * 2, 0xffffffffu);
    for (uint32_t i = 0; i < G; ++i) {
        const uint32_t g = order[i];
        if (g >= G || h[g] != 0xffffffffu) { set_error("the order is not a permutation of the %u local genomes (entry %u: %u)", G, i, g); return MK_ERR_ARG; }
        h[g] = i;
        h[(size_t)G + i] = g;
    }
    MK_TRY(need_raw_cold(c));                                     // (the rule the exports follow: packed cold rows are unpacked first)
    uint32_t *d_buf = nullptr;
    MK_TRY(dev_alloc(&d_buf, (uint64_t)G * 3));
    DevGuard<uint32_t> guard(d_buf);
    MK_HIP(hipMemcpyAsync(d_buf, h.data(), (size_t)G * 8, hipMemcpyHostToDevice, c->stream));
    MK_HIP(hipMemsetAsync(d_buf + (size_t)G * 2, 0, (size_t)G * 4, c->stream));
    {
        ScopedTimer t(c, 2);
        MK_TRY(launch_cover_win(c, d_seen, d_buf, d_buf + G, d_buf + (size_t)G * 2));
    }
    std::vector<uint32_t> got(G);                                 // (a failure after this point leaves `won` as it was)
    MK_HIP(hipMemcpyAsync(got.data(), d_buf + (size_t)G * 2, (size_t)G * 4, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    uint64_t sum = 0;
    for (uint32_t g = 0; g < G; ++g) sum += won[g] = got[g];
    if (claimed) *claimed = sum;
    return drain_timers(c);
}

int mk_cover_winners(mk_ctx *c, const uint32_t *d_seen, uint32_t *covered, uint32_t *won, uint64_t *cells, uint64_t *claimed)
{
    if (!c || !d_seen) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G;
    if (G && (!covered || !won)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(cover_win_values(c, nullptr));                         // (before the count pass writes anything)
    MK_TRY(mk_cover_count(c, d_seen, covered, cells));
    if (!G) { if (claimed) *claimed = 0; return MK_OK; }
    std::vector<uint32_t> order(G);
    cover_order(covered, c->h_sketch_size.data(), G, order.data(), nullptr);
    return mk_cover_assign(c, d_seen, order.data(), won, claimed);
}

int mk_query_cover_winners(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t *covered, uint32_t *won,
                           uint64_t *cells, uint64_t *claimed)
{
    if (!c || (nq && (!seqs || !lens))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (!c->G) { if (cells) *cells = 0; if (claimed) *claimed = 0; return MK_OK; }
    if (!covered || !won) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(cover_win_values(c, nullptr));
    uint32_t *d_seen = nullptr;
    MK_TRY(table_alloc(&d_seen, cover_table_bytes(c)));
    DevGuard<uint32_t> guard(d_seen);
    MK_TRY(mark_uploaded(c, seqs, lens, nq, d_seen, nullptr));
    return mk_cover_winners(c, d_seen, covered, won, cells, claimed);           // (waits: the table goes when this returns)
}

}  // extern "C"

// ---- taxon cover: per node of a taxonomy the distinct cells its genomes hold and those of them the table has seen
// (taxcover.hip).  The nodes of one genome from sketch_size and the plain count pass, every other node from the node pass over
// a work list made here.
extern "C" {

int mk_taxonomy_cover(mk_ctx *c, const mk_taxonomy *tax, const uint32_t *d_seen, mk_node_cover *out, uint64_t *cells)
{
    if (!c || !tax || (tax->n_nodes && !out)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    MK_TRY(genome_map_owned(c, tax->leaf));
    uint32_t rows = 0, wide = 0, ntiles = 0;
    MK_TRY(taxcover_switches(c, &rows, &wide));
    MK_TRY(genome_map_fresh(c, tax->leaf));
    const uint32_t n_nodes = tax->n_nodes, G = c->G;
    std::vector<TaxItem> items;
    bool singles = false;
    if (n_nodes && G) {
        MK_TRY(row_tiles(c, &ntiles));                            // (the segments' 16-byte pieces lie inside whole tiles)
        MK_TRY(taxcover_items(c, tax->lo.data(), tax->hi.data(), n_nodes, rows, wide, items));
        for (uint32_t v = 0; v < n_nodes && !singles; ++v) singles = tax->hi[v] - tax->lo[v] == 1;
    }
    MK_TRY(need_raw_cold(c));                                     // (the rule the exports follow: packed cold rows are unpacked first)
    const bool count = singles && d_seen;                         // the plain count pass, for the nodes of one genome
    // 8-byte words: [cells][out: n_nodes x 2][items: n_items x 2][covered: G 32-bit words]
    const uint64_t n_items = items.size(), words = 1 + (uint64_t)n_nodes * 2 + n_items * 2 + (count ? ((uint64_t)G + 1) / 2 : 0);
    unsigned long long *d_buf = nullptr;
    MK_TRY(dev_alloc(&d_buf, words));
    DevGuard<unsigned long long> guard(d_buf);
    mk_node_cover *d_out = reinterpret_cast<mk_node_cover *>(d_buf + 1);
    TaxItem *d_items = reinterpret_cast<TaxItem *>(d_buf + 1 + (uint64_t)n_nodes * 2);
    uint32_t *d_cov = reinterpret_cast<uint32_t *>(d_buf + 1 + (uint64_t)n_nodes * 2 + n_items * 2);
    MK_HIP(hipMemsetAsync(d_buf, 0, words * 8, c->stream));
    // (from pageable memory: the host waits until the stream has reached the copy, so the list is free on return)
    if (n_items) MK_HIP(hipMemcpyAsync(d_items, items.data(), (size_t)n_items * sizeof(TaxItem), hipMemcpyHostToDevice, c->stream));
    {
        ScopedTimer t(c, 2);
        MK_TRY(launch_taxcover(c, d_items, (uint32_t)n_items, tax->d_lo, tax->d_hi, d_seen, d_out));
        if (d_seen && (count || cells)) MK_TRY(launch_cover_count(c, d_seen, count ? d_cov : nullptr, cells ? d_buf : nullptr));
    }
    std::vector<mk_node_cover> got(n_nodes);                      // (a failure after this point leaves `out` as it was)
    std::vector<uint32_t> cov(count ? G : 0);
    uint64_t n_cells = 0;
    if (n_nodes) MK_HIP(hipMemcpyAsync(got.data(), d_out, (size_t)n_nodes * sizeof(mk_node_cover), hipMemcpyDeviceToHost, c->stream));
    if (count) MK_HIP(hipMemcpyAsync(cov.data(), d_cov, (size_t)G * 4, hipMemcpyDeviceToHost, c->stream));
    if (cells) MK_HIP(hipMemcpyAsync(&n_cells, d_buf, 8, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t v = 0; v < n_nodes; ++v) {
        if (tax->hi[v] - tax->lo[v] == 1) got[v] = mk_node_cover{c->h_sketch_size[tax->lo[v]], count ? cov[tax->lo[v]] : 0u};
        out[v] = got[v];
    }
    if (cells) *cells = n_cells;
    return drain_timers(c);
}

int mk_query_taxonomy_cover(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, const uint32_t *lo, const uint32_t *hi,
                            uint32_t n_nodes, mk_node_cover *out, uint64_t *cells)
{
    if (!c || (nq && (!seqs || !lens))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (!c->G) { if (cells) *cells = 0; return MK_OK; }
    if (n_nodes && (!lo || !hi || !out)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(taxcover_switches(c, nullptr, nullptr));               // (refused here, before anything is uploaded)
    mk_taxonomy *made = nullptr;
    MK_TRY(taxonomy_make(c, lo, hi, n_nodes, c->G, &made));
    std::unique_ptr<mk_taxonomy> tax(made);                        // (goes on return: the pass has waited)
    uint32_t *d_seen = nullptr;
    MK_TRY(table_alloc(&d_seen, cover_table_bytes(c)));
    DevGuard<uint32_t> guard(d_seen);
    MK_TRY(mark_uploaded(c, seqs, lens, nq, d_seen, nullptr));
    return mk_taxonomy_cover(c, tax.get(), d_seen, out, cells);   // (waits: the table goes when this returns)
}

}  // extern "C"

// ---- taxon markers: every held cell credited to the deepest node of a taxonomy that contains all its holders, and those of a
// node's own cells the table has seen (markers.hip): one pass, n_nodes + 1 pairs of counters zeroed, added to, copied out.
extern "C" {

int mk_taxonomy_markers(mk_ctx *c, const mk_taxonomy *tax, const uint32_t *d_seen, mk_node_markers *out, uint32_t n_slots, uint64_t *cells)
{
    if (!c || !tax || !out) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    MK_TRY(genome_map_owned(c, tax->leaf));
    if ((uint64_t)n_slots < (uint64_t)tax->n_nodes + 1) { set_error("the taxonomy has %u nodes and the slot above them, beyond the counters' %u slots", tax->n_nodes, n_slots); return MK_ERR_ARG; }
    MK_TRY(markers_switches(c, nullptr, nullptr, nullptr));
    MK_TRY(genome_map_fresh(c, tax->leaf));
    const uint32_t n_nodes = tax->n_nodes;
    MK_TRY(need_raw_cold(c));                                     // (the rule the exports follow: packed cold rows are unpacked first)
    // 8-byte words: [cells][out: (n_nodes + 1) x 2]
    const uint64_t words = 1 + ((uint64_t)n_nodes + 1) * 2;
    unsigned long long *d_buf = nullptr;
    MK_TRY(dev_alloc(&d_buf, words));
    DevGuard<unsigned long long> guard(d_buf);
    mk_node_markers *d_out = reinterpret_cast<mk_node_markers *>(d_buf + 1);
    MK_HIP(hipMemsetAsync(d_buf, 0, words * 8, c->stream));
    {
        ScopedTimer t(c, 2);
        MK_TRY(launch_markers(c, tax->leaf.d_word, tax->d_parent, tax->d_hi, tax->d_live, tax->leaf.n, n_nodes, d_seen, d_out));
        if (d_seen && cells) MK_TRY(launch_cover_count(c, d_seen, nullptr, d_buf));
    }
    std::vector<mk_node_markers> got((size_t)n_nodes + 1);        // (a failure after this point leaves `out` as it was)
    uint64_t n_cells = 0;
    MK_HIP(hipMemcpyAsync(got.data(), d_out, got.size() * sizeof(mk_node_markers), hipMemcpyDeviceToHost, c->stream));
    if (cells) MK_HIP(hipMemcpyAsync(&n_cells, d_buf, 8, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    std::copy(got.begin(), got.end(), out);
    if (cells) *cells = n_cells;
    return drain_timers(c);
}

int mk_query_taxonomy_markers(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, const uint32_t *lo, const uint32_t *hi,
                              uint32_t n_nodes, mk_node_markers *out, uint32_t n_slots, uint64_t *cells)
{
    if (!c || !out || (nq && (!seqs || !lens)) || (n_nodes && (!lo || !hi))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if ((uint64_t)n_slots < (uint64_t)n_nodes + 1) { set_error("the taxonomy has %u nodes and the slot above them, beyond the counters' %u slots", n_nodes, n_slots); return MK_ERR_ARG; }
    MK_TRY(markers_switches(c, nullptr, nullptr, nullptr));       // (refused here, before anything is uploaded)
    if (!c->G) { out[0] = mk_node_markers{0, 0}; if (cells) *cells = 0; return MK_OK; }
    mk_taxonomy *made = nullptr;
    MK_TRY(taxonomy_make(c, lo, hi, n_nodes, c->G, &made));
    std::unique_ptr<mk_taxonomy> tax(made);                        // (goes on return: the pass has waited)
    uint32_t *d_seen = nullptr;
    MK_TRY(table_alloc(&d_seen, cover_table_bytes(c)));
    DevGuard<uint32_t> guard(d_seen);
    MK_TRY(mark_uploaded(c, seqs, lens, nq, d_seen, nullptr));
    return mk_taxonomy_markers(c, tax.get(), d_seen, out, n_slots, cells);   // (waits: the table goes when this returns)
}

}  // extern "C"

// ---- depth: the gated sketch of a set added, saturating at 255, into a table of (partition, value) bytes, and nine passes
// over the matrix that give per genome the covered fingerprints, the sum and the median of their bytes (depth.hip).  The
// set is taken as the cover takes it (qset_mark): its sketch only, a prepared set keeps what it has.
extern "C" {

uint64_t mk_depth_bytes(const mk_ctx *c) { return c ? depth_table_bytes(c) : 0; }

int mk_depth_reset(mk_ctx *c, uint8_t *d_mult)
{
    if (!c || !d_mult) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return launch_depth_reset(c, d_mult);
}

int mk_qset_run_depth(mk_ctx *c, mk_qset *qs, uint8_t *d_mult)
{
    if (!c || !qs || !d_mult) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return qset_mark(c, qs, [&](const mk_qset *leaf) { return launch_depth_mark(c, leaf, d_mult); });
}

int mk_depth_profile(mk_ctx *c, const uint8_t *d_mult, mk_depth *depth, uint64_t *cells, uint64_t *saturated)
{
    if (!c || !d_mult) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G;
    if (G && !depth) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(need_raw_cold(c));                                     // (the rule the exports follow: packed cold rows are unpacked first)
    // [cells, saturated: 8 bytes each][depth: G x 16 bytes][the passes' scratch], 8-byte words
    const uint64_t words = 2 + (uint64_t)G * 2 + (depth_scratch_words(G) + 1) / 2;
    unsigned long long *d_out = nullptr;
    MK_TRY(dev_alloc(&d_out, words));
    DevGuard<unsigned long long> guard(d_out);
    mk_depth *d_depth = reinterpret_cast<mk_depth *>(d_out + 2);
    MK_HIP(hipMemsetAsync(d_out, 0, 16, c->stream));
    {
        ScopedTimer t(c, 2);
        MK_TRY(launch_depth_profile(c, d_mult, reinterpret_cast<uint32_t *>(d_out + 2 + (size_t)G * 2), d_depth));
        if (cells || saturated) MK_TRY(launch_depth_cells(c, d_mult, d_out));
    }
    std::vector<mk_depth> got(G);                                 // (a failure after this point leaves `depth` as it was)
    uint64_t totals[2] = {0, 0};
    if (G) MK_HIP(hipMemcpyAsync(got.data(), d_depth, (size_t)G * sizeof(mk_depth), hipMemcpyDeviceToHost, c->stream));
    if (cells || saturated) MK_HIP(hipMemcpyAsync(totals, d_out, 16, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (G) std::copy(got.begin(), got.end(), depth);
    if (cells) *cells = totals[0];
    if (saturated) *saturated = totals[1];
    return drain_timers(c);
}

int mk_query_depth(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, mk_depth *depth, uint64_t *cells, uint64_t *saturated)
{
    if (!c || (nq && (!seqs || !lens))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (!c->G) { if (cells) *cells = 0; if (saturated) *saturated = 0; return MK_OK; }
    if (!depth) { set_error("null argument"); return MK_ERR_ARG; }
    uint8_t *d_mult = nullptr;
    MK_TRY(table_alloc(&d_mult, depth_table_bytes(c)));
    DevGuard<uint8_t> guard(d_mult);
    MK_TRY(mark_uploaded(c, seqs, lens, nq, nullptr, d_mult));
    return mk_depth_profile(c, d_mult, depth, cells, saturated);                // (waits: the table goes when this returns)
}

}  // extern "C"

// ---- panel: up to eight samples' gated sketches OR-ed into the bits of a table of (partition, value) bytes, and ONE pass over
// the matrix that counts per slot and genome the stored fingerprints the slot's plane holds (panel.hip).  A set is taken as the
// cover takes it (qset_mark).
extern "C" {

uint64_t mk_panel_bytes(const mk_ctx *c) { return c ? panel_table_bytes(c) : 0; }

int mk_panel_reset(mk_ctx *c, uint8_t *d_panel)
{
    if (!c || !d_panel) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return launch_panel_reset(c, d_panel);
}

int mk_qset_run_panel(mk_ctx *c, mk_qset *qs, uint32_t slot, uint8_t *d_panel)
{
    if (!c || !qs || !d_panel) { set_error("null argument"); return MK_ERR_ARG; }
    if (slot >= MK_PANEL_SLOTS) { set_error("panel slot %u: a panel has %u slots", slot, MK_PANEL_SLOTS); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return qset_mark(c, qs, [&](const mk_qset *leaf) { return launch_panel_mark(c, leaf, slot, d_panel); });
}

int mk_panel_count(mk_ctx *c, const uint8_t *d_panel, uint32_t n_slots, uint32_t *covered, uint64_t *cells)
{
    if (!c || !d_panel) { set_error("null argument"); return MK_ERR_ARG; }
    if (!n_slots || n_slots > MK_PANEL_SLOTS) { set_error("a panel count of %u slots: a panel has 1 to %u", n_slots, MK_PANEL_SLOTS); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G;
    if (G && !covered) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(need_raw_cold(c));                                     // (the rule the exports follow: packed cold rows are unpacked first)
    // [cells: 8 x 8 bytes][covered: n_slots x G words], zeroed, added to by the kernels, copied out
    const size_t words = 2 * (size_t)MK_PANEL_SLOTS + (size_t)n_slots * G;
    uint32_t *d_out = nullptr;
    MK_TRY(dev_alloc(&d_out, (uint64_t)words));
    DevGuard<uint32_t> guard(d_out);
    MK_HIP(hipMemsetAsync(d_out, 0, words * 4, c->stream));
    {
        ScopedTimer t(c, 2);
        MK_TRY(launch_panel_count(c, d_panel, n_slots, G ? d_out + 2 * MK_PANEL_SLOTS : nullptr, cells ? reinterpret_cast<unsigned long long *>(d_out) : nullptr));
    }
    if (G) MK_HIP(hipMemcpyAsync(covered, d_out + 2 * MK_PANEL_SLOTS, (size_t)n_slots * G * 4, hipMemcpyDeviceToHost, c->stream));
    if (cells) MK_HIP(hipMemcpyAsync(cells, d_out, (size_t)n_slots * 8, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    return drain_timers(c);
}

int mk_panel_slot(mk_ctx *c, const uint8_t *d_panel, uint32_t slot, uint32_t *d_seen)
{
    if (!c || !d_panel || !d_seen) { set_error("null argument"); return MK_ERR_ARG; }
    if (slot >= MK_PANEL_SLOTS) { set_error("panel slot %u: a panel has %u slots", slot, MK_PANEL_SLOTS); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return launch_panel_slot(c, d_panel, slot, d_seen);
}

int mk_query_panel(mk_ctx *c, const char *const *seqs, const uint64_t *lens, const uint64_t *starts, uint32_t n_samples, uint32_t *covered,
                   uint64_t *cells)
{
    if (!c || !starts) { set_error("null argument"); return MK_ERR_ARG; }
    if (starts[0] != 0) { set_error("the samples' starts begin at %llu, not at 0", (unsigned long long)starts[0]); return MK_ERR_ARG; }
    for (uint32_t s = 0; s < n_samples; ++s)
        if (starts[s + 1] < starts[s]) { set_error("the samples' starts decrease at sample %u", s); return MK_ERR_ARG; }
    if (starts[n_samples] && (!seqs || !lens)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G;
    if (!n_samples || !G) {
        if (cells) std::fill(cells, cells + n_samples, 0);
        return MK_OK;
    }
    if (!covered) { set_error("null argument"); return MK_ERR_ARG; }
    uint8_t *d_panel = nullptr;
    MK_TRY(table_alloc(&d_panel, panel_table_bytes(c)));
    DevGuard<uint8_t> guard(d_panel);
    constexpr uint64_t kMaxPiece = 1ull << 30;                    // (for_uploaded_slices counts in 32 bits)
    for (uint32_t s0 = 0; s0 < n_samples; s0 += MK_PANEL_SLOTS) {
        const uint32_t n = std::min(MK_PANEL_SLOTS, n_samples - s0);
        MK_TRY(launch_panel_reset(c, d_panel));
        for (uint32_t slot = 0; slot < n; ++slot)
            for (uint64_t q0 = starts[s0 + slot], q1 = starts[s0 + slot + 1]; q0 < q1; q0 += kMaxPiece) {
                // (in slices: an OR leaves no trace of the slicing)
                MK_TRY(for_uploaded_slices(c, seqs + q0, lens + q0, (uint32_t)std::min(kMaxPiece, q1 - q0), [&](mk_qset *qs, uint32_t, uint32_t) {
                    return qset_mark(c, qs, [&](const mk_qset *leaf) { return launch_panel_mark(c, leaf, slot, d_panel); });
                }));
            }
        MK_TRY(mk_panel_count(c, d_panel, n, covered + (size_t)s0 * G, cells ? cells + s0 : nullptr));   // (waits)
    }
    return MK_OK;                                                 // (the table goes when this returns: the last count has waited)
}

}  // extern "C"

// ---- gather: the greedy set cover over a cover table (gather.hip): the count pass once, then rounds of pick, take and strike
// on a copy of the table, queued several at a time; the host reads the rounds' 24-byte records and the `done` flag between the
// batches and nothing else.
extern "C" {

int mk_cover_gather(mk_ctx *c, const uint32_t *d_seen, const uint8_t *d_mult, uint32_t min_new, uint32_t max_picks, mk_pick *picks,
                    uint32_t *n_picks, uint64_t *cells, uint64_t *explained)
{
    if (!c || !d_seen || !n_picks) { set_error("null argument"); return MK_ERR_ARG; }
    if (!min_new) { set_error("min_new = 0: every genome would be picked, the last ones for nothing; the least is 1"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G, P = c->P;
    if (!G) {
        uint64_t n = 0;
        if (cells) MK_TRY(mk_cover_count(c, d_seen, nullptr, &n));
        if (cells) *cells = n;
        *n_picks = 0;
        if (explained) *explained = 0;
        return MK_OK;
    }
    if (!picks) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(need_raw_cold(c));                                     // (the rule the exports follow: packed cold rows are unpacked first)
    const uint32_t rounds = max_picks ? std::min(max_picks, G) : G;
    const uint64_t bytes = cover_table_bytes(c);
    uint32_t *d_live = nullptr;
    MK_TRY(table_alloc(&d_live, bytes));                          // (out of memory: MK_ERR_NOMEM, nothing written)
    DevGuard<uint32_t> guard_live(d_live);
    // 8-byte words: [cells][done][slots: rounds][records: rounds x 3][strike list: P][rem: G 32-bit words]
    const uint64_t words = 2 + (uint64_t)rounds * 4 + P + ((uint64_t)G + 1) / 2;
    unsigned long long *d_state = nullptr;
    if (hipMalloc((void **)&d_state, words * 8) != hipSuccess) {
        (void)hipGetLastError();
        set_error("out of device memory (%llu bytes of gather state)", (unsigned long long)(words * 8));
        return MK_ERR_NOMEM;
    }
    DevGuard<unsigned long long> guard_state(d_state);
    GatherArgs a;
    a.live = d_live;
    a.mult = d_mult;
    a.done = reinterpret_cast<uint32_t *>(d_state + 1);
    a.slots = d_state + 2;
    a.recs = reinterpret_cast<mk_pick *>(d_state + 2 + rounds);
    a.list = reinterpret_cast<uint64_t *>(d_state + 2 + (uint64_t)rounds * 4);
    a.rem = reinterpret_cast<uint32_t *>(d_state + 2 + (uint64_t)rounds * 4 + P);
    a.min_new = min_new;
    a.cap = rounds;
    a.recount = gather_recount();
    const uint32_t per_wait = gather_rounds_per_wait();
    MK_HIP(hipMemcpyAsync(d_live, d_seen, bytes, hipMemcpyDeviceToDevice, c->stream));
    MK_HIP(hipMemsetAsync(d_state, 0, words * 8, c->stream));
    {
        ScopedTimer t(c, 2);
        MK_TRY(launch_cover_count(c, d_live, a.rem, d_state));
    }
    std::vector<uint32_t> rem0(G);
    uint64_t n_cells = 0;
    MK_HIP(hipMemcpyAsync(rem0.data(), a.rem, (size_t)G * 4, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipMemcpyAsync(&n_cells, d_state, 8, hipMemcpyDeviceToHost, c->stream));
    std::vector<mk_pick> got;                                     // (a failure leaves the outputs as they were)
    std::vector<mk_pick> batch(std::min(per_wait, rounds));
    uint64_t sum = 0;
    bool stopped = false;
    for (uint32_t r = 0; r < rounds && !stopped;) {
        const uint32_t n = std::min(per_wait, rounds - r);
        {
            ScopedTimer t(c, 2);
            for (uint32_t i = 0; i < n; ++i) MK_TRY(launch_gather_round(c, a, r + i));
        }
        uint32_t done = 0;
        MK_HIP(hipMemcpyAsync(batch.data(), a.recs + r, (size_t)n * sizeof(mk_pick), hipMemcpyDeviceToHost, c->stream));
        MK_HIP(hipMemcpyAsync(&done, a.done, 4, hipMemcpyDeviceToHost, c->stream));
        MK_HIP(hipStreamSynchronize(c->stream));
        for (uint32_t i = 0; i < n && !stopped; ++i) {
            mk_pick x = batch[i];
            if (x.fresh < min_new) { stopped = true; break; }     // (the round that set `done` left its record zero)
            if (x.covered != x.fresh || x.genome >= G || x.fresh > rem0[x.genome]) {
                (void)drain_timers(c);
                set_error("gather: round %u picked genome %u for %u cells and struck %u (it covers %u): the library disagrees with itself",
                          r + i, x.genome, x.fresh, x.covered, x.genome < G ? rem0[x.genome] : 0u);
                return MK_ERR_STATE;
            }
            sum += x.fresh;
            x.covered = rem0[x.genome];
            x.sketch_size = c->h_sketch_size[x.genome];
            x.genome += c->p.genome_id_base;
            got.push_back(x);
        }
        if (stopped != (done != 0)) {
            (void)drain_timers(c);
            set_error("gather: the device's stop flag reads %u after round %u, the records say %s", done, r + n - 1, stopped ? "stopped" : "going on");
            return MK_ERR_STATE;
        }
        r += n;
    }
    MK_HIP(hipStreamSynchronize(c->stream));
    std::copy(got.begin(), got.end(), picks);
    *n_picks = (uint32_t)got.size();
    if (cells) *cells = n_cells;
    if (explained) *explained = sum;
    return drain_timers(c);
}

int mk_query_cover_gather(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, int with_depth, uint32_t min_new,
                          uint32_t max_picks, mk_pick *picks, uint32_t *n_picks, uint64_t *cells, uint64_t *explained)
{
    if (!c || !n_picks || (nq && (!seqs || !lens))) { set_error("null argument"); return MK_ERR_ARG; }
    if (!min_new) { set_error("min_new = 0: every genome would be picked, the last ones for nothing; the least is 1"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (!c->G) { *n_picks = 0; if (cells) *cells = 0; if (explained) *explained = 0; return MK_OK; }
    if (!picks) { set_error("null argument"); return MK_ERR_ARG; }
    uint32_t *d_seen = nullptr;
    uint8_t *d_mult = nullptr;
    MK_TRY(table_alloc(&d_seen, cover_table_bytes(c)));
    DevGuard<uint32_t> guard(d_seen);
    if (with_depth) MK_TRY(table_alloc(&d_mult, depth_table_bytes(c)));
    DevGuard<uint8_t> guard_depth(d_mult);
    MK_TRY(mark_uploaded(c, seqs, lens, nq, d_seen, d_mult));
    return mk_cover_gather(c, d_seen, d_mult, min_new, max_picks, picks, n_picks, cells, explained);   // (waits: the tables go when this returns)
}

}  // extern "C"

// ---- representatives: the list walk with a bitmap row per query as its sink (rep.hip) ------------------------------------
// (the index in sets of ids, as mk_index_families takes it; the resolve step takes a set in pieces of kRepMaxSet ids)
extern "C" {

int mk_index_representatives(mk_ctx *c, uint32_t min_score, double min_inter, uint32_t *rep)
{
    if (!c) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    const uint32_t G = c->G, base = c->p.genome_id_base;
    if (!G) return MK_OK;
    if (!rep) { set_error("null argument"); return MK_ERR_ARG; }
    if ((uint64_t)base + G > 0xffffffffull) { set_error("genome ids beyond 32 bits"); return MK_ERR_ARG; }
    MK_TRY(refuse_nan_lists(c, min_score));
    const uint32_t per = index_set_ids(c), row_words = rep_row_words(G);
    mk_ctx::RepScratch &rs = c->rep;
    MK_HIP(hipStreamSynchronize(c->stream));                       // (an earlier call's launches may still read the scratch)
    MK_TRY(rs.d_rows.grow((uint64_t)std::min(per, G) * row_words));
    MK_TRY(rs.d_rep.grow((uint64_t)G));
    MK_TRY(rs.d_is_rep.grow(((uint64_t)G + 31) / 32));
    {
        ScopedTimer t(c, 2);
        MK_TRY(launch_rep_reset(c, rs.d_rep, G, rs.d_is_rep));
    }
    // (for_index_sets waits for a set's pass before the next: the rows are the next set's)
    MK_TRY(for_index_sets(c, per, [&](mk_qset *qs, const uint32_t *, uint32_t g0, uint32_t n) -> int {
        // the walk pass over the set (its columns as the index holds them: a packed index is unpacked): every chunk's queries
        // write their rows of the set's bitmap
        MK_TRY(qset_leaves(c, qs, [&](mk_qset *leaf, const std::vector<uint32_t> *) {
            return qset_walk(c, leaf, min_score, min_inter, [&](uint32_t q0, const ListArgs &a) { return launch_rep_rows(c, RepRowsArgs{a, q0, g0, rs.d_rows, row_words}); });
        }));
        // the set's bitmap is complete: its ids in order, as many at a time as the resolve step's matrix holds
        for (uint32_t i0 = 0; i0 < n; i0 += kRepMaxSet) {
            ScopedTimer t(c, 2);
            MK_TRY(launch_rep_resolve(c, RepArgs{rs.d_rows + (uint64_t)i0 * row_words, row_words, g0 + i0, std::min(kRepMaxSet, n - i0), G, rs.d_rep, rs.d_is_rep}));
        }
        return MK_OK;
    }));
    MK_HIP(hipMemcpyAsync(rep, rs.d_rep, (size_t)G * 4, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t j = 0; j < G; ++j) rep[j] += base;
    return drain_timers(c);
}

}  // extern "C"
