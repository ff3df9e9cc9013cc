// Building and editing the index of the `miekki` binary: -l (index_file_of_file, in one process or one per GPU), -K, and
//   * -M <file> (not in the reference, whose merge_indexes is unfinished): the genomes of another index file behind those of
//     -i, as if both had been built as one list (join_index below).  Repeatable, applied in order; needs -i; one GPU.
#include "driver.hpp"

#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <deque>
#include <future>
#include <thread>
#include <unordered_map>

#include "index_io.hpp"

using namespace std;

namespace mkhost {

namespace {

// A unit's files go to the device as the readers read them (RawSink -> mk_gz_open / mk_gz_stage / mk_gz_put): straight
// from the page cache into page-locked pieces the library lends, a DMA each, into a batch whose layout the files'
// sizes fixed -- nothing of a gzip'd file waits in host memory.  A unit the device has no memory for is the readers'.
// A unit RUNS (mk_gz_run, on a thread of its own) as soon as its last file has been put -- the reader that put it says
// so -- not when this thread gets round to it: the device inflates the units ahead while the ones before them are
// being appended.
struct UnitRun { std::future<int> ran; string error; };
struct Sink {
    mk_ctx *ctx;
    std::mutex m;
    std::unordered_map<void *, std::shared_ptr<UnitRun>> runs;
    static void *open(void *u, const uint64_t *sizes, uint32_t m, uint64_t *offsets)
    {
        mk_gz_batch *b = nullptr;
        if (mk_gz_open(((Sink *)u)->ctx, sizes, m, &b) != MK_OK) return nullptr;
        if (mk_gz_layout(b, offsets) != MK_OK) { mk_gz_free(b); return nullptr; }
        return b;
    }
    static bool put_span(void *, void *batch, uint32_t first, uint32_t count, const void *data, uint64_t bytes, bool staged)
    {
        return mk_gz_put_span((mk_gz_batch *)batch, first, count, data, bytes, staged ? 1 : 0) == MK_OK;
    }
    static void *stage(void *, void *batch, uint64_t *cap) { return mk_gz_stage((mk_gz_batch *)batch, cap); }
    static bool put(void *, void *batch, uint32_t i, uint64_t at, const void *data, uint64_t bytes, bool staged)
    {
        return mk_gz_put((mk_gz_batch *)batch, i, at, data, bytes, staged ? 1 : 0) == MK_OK;
    }
    static void complete(void *u, void *batch)
    {
        std::shared_ptr<UnitRun> r = std::make_shared<UnitRun>();
        UnitRun *rp = r.get();
        r->ran = std::async(std::launch::async, [rp, batch]() -> int {
            const int rc = mk_gz_run((mk_gz_batch *)batch);
            if (rc != MK_OK) rp->error = mk_last_error();
            return rc;
        });
        std::lock_guard<std::mutex> g(((Sink *)u)->m);
        ((Sink *)u)->runs[batch] = std::move(r);
    }
    std::shared_ptr<UnitRun> take(void *batch)
    {
        std::lock_guard<std::mutex> g(m);
        auto it = runs.find(batch);
        if (it == runs.end()) return nullptr;
        std::shared_ptr<UnitRun> r = std::move(it->second);
        runs.erase(it);
        return r;
    }
    ~Sink() { for (auto &kv : runs) if (kv.second && kv.second->ran.valid()) (void)kv.second->ran.get(); }
};

// What has been taken from the readers and waits for its turn, in list order: runs of up to 64 sequences the readers
// made (packed), and whole UNITS that went to the device -- each run by a thread of its own (mk_gz_run works on a
// stream of its own; a deflate stream is decoded by few lanes, so it is batches side by side that fill the device).
// Everything is appended in list order, sixty-four at a time.
struct Pending {
    vector<OrderedFastaReader::Item> items;
    vector<string> names;
    mk_gz_batch *batch = nullptr;                           // a device unit: its files' bytes are there already
    std::shared_ptr<UnitRun> run;                           // ... and it runs, or has run (the readers started it)
};

// (whatever way this function is left: no thread of a batch still runs, no batch keeps its blocks)
struct Cleanup {
    std::deque<std::unique_ptr<Pending>> &pending; std::unique_ptr<Pending> &cur;
    ~Cleanup()
    {
        auto drop = [](Pending *p) { if (!p) return; if (p->run && p->run->ran.valid()) (void)p->run->ran.get(); if (p->batch && p->run) mk_gz_free(p->batch); p->batch = nullptr; };
        for (auto &p : pending) drop(p.get());
        drop(cur.get());
    }
};

}  // namespace

// one shard's share of index_file_of_file: files [f0, f1) of the list into ctx, in order.
// `log` collects what the reference prints meanwhile (one '-' per genome kept, the
// "Missed file" lines) so that several shards' output can be shown in list order.
void Driver::build_shard(mk_ctx *ctx, const vector<string> &files, unsigned nthreads, bool live, ShardBuild &sb)
{
    const double t_enter = chrono::duration<double>(chrono::steady_clock::now().time_since_epoch()).count();
    // a doubling matrix would hold old and new copy at once: size it for the whole list up front
    if (!files.empty() && mk_reserve(ctx, (uint32_t)files.size()) != MK_OK) { sb.error = string("index build failed: ") + mk_last_error(); return; }
    // readers parse into pinned buffers, three device batches ahead; the append of one
    // batch returns as soon as its copy is done, so parsing, copying and sketching overlap
    // ... and pack as they parse (2 bits per base, mk_index_append_packed): a quarter of the bytes to buffer and
    // to move over PCIe, and the device skips its own packing pass.
    // gzip'd files -- the reference's normal input (zstr, Miekki.cpp:559) -- arrive as their bytes and are inflated,
    // stripped and appended on the device, a few thousand at a time (a deflate stream is decoded by one lane, so it is
    // the number of streams in flight that makes the rate; MIEKKI_GZ_BATCH sets it, 0 = the readers inflate);
    // whatever the device refuses is inflated here
    // the list goes to the device in units of 512 files, three of them ahead of this thread (fixed: what was measured is in
    // profiles/r6_ingest_gz.txt; a -DMK_TUNE_BUILD binary reads MIEKKI_GZ_BATCH -- 0: the readers inflate everything --,
    // MIEKKI_GZ_IN_FLIGHT, and MIEKKI_GZ_SHARE=1: the readers' own zlib takes a unit whenever three are waiting at the device)
#ifdef MK_TUNE_BUILD
    static const size_t gz_batch = [] { const char *e = getenv("MIEKKI_GZ_BATCH"); return e ? (size_t)std::max(0L, atol(e)) : (size_t)512; }();
    static const size_t gz_in_flight = [] { const char *e = getenv("MIEKKI_GZ_IN_FLIGHT"); return e ? (size_t)std::max(1L, atol(e)) : (size_t)3; }();
    static const bool gz_share = [] { const char *e = getenv("MIEKKI_GZ_SHARE"); return e && atoi(e) != 0; }();
#else
    constexpr size_t gz_batch = 512, gz_in_flight = 3;
    constexpr bool gz_share = false;
#endif
    Sink sink_user;                                              // (the units the readers started: see Sink)
    sink_user.ctx = ctx;
    mkhost::RawSink sink;
    sink.user = &sink_user; sink.open = Sink::open; sink.stage = Sink::stage; sink.put = Sink::put; sink.put_span = Sink::put_span; sink.complete = Sink::complete;
    // (the arena outlives the reader: declared first.  Both are handed to a thread of their own when the shard is built:
    // giving gigabytes of page-locked memory back takes tenths of a second that nothing has to wait for)
    std::shared_ptr<PinnedArena> arena_p = std::make_shared<PinnedArena>(ctx);
    std::unique_ptr<OrderedFastaReader> reader_p(new OrderedFastaReader(files, nthreads, mkhost::HostAllocator{pinned_alloc, pinned_free, arena_p.get()},
                                                                        std::max<size_t>(3 * 64, gz_in_flight * gz_batch + 64), true, gz_batch != 0,
                                                                        gz_batch, gz_in_flight, gz_batch ? sink : mkhost::RawSink(), gz_share));
    OrderedFastaReader &reader = *reader_p;
    auto now = [] { return chrono::duration<double>(chrono::steady_clock::now().time_since_epoch()).count(); };
    auto show = [&]() { if (live) { cout << sb.log << flush_stream(); sb.log.clear(); } };
    std::deque<std::unique_ptr<Pending>> pending;
    size_t raw_in_flight = 0, host_waiting = 0;
    std::unique_ptr<Pending> cur;                               // the run being collected
    uint64_t cur_bytes = 0;
    Cleanup cleanup{pending, cur};
    auto close_run = [&]() {
        if (!cur) return;
        if (cur->batch) {
            cur->run = sink_user.take(cur->batch);                // (started when the unit's last file had been put: before its item could be taken)
            ++raw_in_flight;
        } else {
            host_waiting += cur->items.size();
        }
        pending.push_back(std::move(cur));
        cur_bytes = 0;
    };
    auto append_items = [&](const OrderedFastaReader::Item *items, size_t n) {      // sequences the readers made, one call
        const double t0 = now();
        int rc;
        if (items[0].packed) {
            vector<mk_packed_seq> p(n);
            for (size_t i = 0; i < n; ++i) {
                p[i].codes = items[i].codes; p[i].except = items[i].dirty ? items[i].except : nullptr; p[i].len = items[i].len;
                memcpy(p[i].head, items[i].head, 32);
            }
            rc = mk_index_append_packed(ctx, p.data(), (uint32_t)n);
        } else {
            vector<const char *> p;
            vector<uint64_t> l;
            for (size_t i = 0; i < n; ++i) { p.push_back(items[i].data); l.push_back(items[i].len); }
            rc = mk_index_append(ctx, p.data(), l.data(), (uint32_t)n);
        }
        if (rc != MK_OK) { sb.error = string("index build failed: ") + mk_last_error(); return false; }
        sb.t_append += now() - t0;
        return true;
    };
    auto append_host_run = [&](Pending &run) {
        if (!append_items(run.items.data(), run.items.size())) return false;
        sb.names.insert(sb.names.end(), run.names.begin(), run.names.end());
        sb.log.append(run.items.size(), '-');
        host_waiting -= run.items.size();
        sb.from_readers += run.items.size();
        for (auto &s : run.items) reader.recycle(s);
        return true;
    };
    // a file the device did not take (or a whole unit it failed on): read and inflated here, appended in its place
    auto append_from_disk = [&](const string &fn) {
        vector<char> text, scratch, seq;
        if (!mkhost::read_file(fn, text, scratch)) { sb.error = "cannot read " + fn; return false; }
        seq.resize(text.size() + 1);
        seq.resize(mkhost::strip_fasta(text.data(), text.size(), seq.data()));
        ++sb.gz_on_host;
        if (seq.size() < k) return true;
        const char *p = seq.data();
        const uint64_t l = seq.size();
        if (mk_index_append(ctx, &p, &l, 1) != MK_OK) { sb.error = string("index build failed: ") + mk_last_error(); return false; }
        sb.names.push_back(fn); sb.log += '-';
        return true;
    };
    mk_gz_batch *retired = nullptr;                              // the unit appended last: its text may still be read
    struct Retire { mk_gz_batch *&b; ~Retire() { if (b) mk_gz_free(b); b = nullptr; } } retire{retired};
    auto append_unit = [&](Pending &rb) {
        const double t0 = now();
        const int ran = rb.run ? rb.run->ran.get() : MK_ERR_STATE;
        sb.t_unpack_wait += now() - t0;
        --raw_in_flight;
        // (a batch the device could not run -- no memory for its text, say -- is read again and inflated here, file by
        // file: slower, never wrong; its blocks go back first)
        if (ran != MK_OK) { mk_gz_free(rb.batch); rb.batch = nullptr; }
        vector<uint32_t> which;                                // files of the batch waiting to be appended together
        vector<string> kept;
        bool ok = true;
        auto append = [&]() {
            if (which.empty()) return true;
            const double ta = now();
            if (mk_index_append_gz(ctx, rb.batch, which.data(), (uint32_t)which.size()) != MK_OK) { sb.error = string("index build failed: ") + mk_last_error(); return false; }
            sb.t_append += now() - ta;
            sb.names.insert(sb.names.end(), kept.begin(), kept.end());
            which.clear(); kept.clear();
            return true;
        };
        for (size_t i = 0; i < rb.items.size() && ok; ++i) {
            OrderedFastaReader::Item &it = rb.items[i];
            if (!it.exists) { ok = append(); sb.log += "Missed file: " + rb.names[i] + "\n"; show(); continue; }
            if (it.failed) { ok = append(); if (ok) { sb.error = "cannot read " + rb.names[i]; ok = false; } break; }
            if (!it.raw) {                                     // a file of the unit that came the ordinary way (not gzip'd after all)
                if (it.len >= k) {
                    ok = append() && append_items(&it, 1);
                    if (ok) { sb.names.push_back(rb.names[i]); sb.log += '-'; ++sb.from_readers; }
                }
                continue;
            }
            uint64_t len = 0;
            int32_t st = MK_GZ_INTERNAL;
            if (rb.batch) mk_gz_sequence(rb.batch, it.unit_index, &len, &st);
            if (st != MK_GZ_OK) { ok = append() && append_from_disk(rb.names[i]); continue; }
            if (len >= k) {
                which.push_back(it.unit_index); kept.push_back(rb.names[i]);
                sb.log += '-';
                if (which.size() >= 64) { ok = append(); show(); }
            }
        }
        ok = ok && append();
        // the batch goes when the NEXT unit has been appended (mk_gz_free waits for the strip kernels that read its text:
        // by then they are long done, and this thread has queued the next appends instead of standing here)
        const double tf = now();
        if (retired) mk_gz_free(retired);
        retired = rb.batch;
        rb.batch = nullptr;
        sb.t_free += now() - tf;
        sb.gz_on_device += rb.items.size();
        const double tr = now();
        for (auto &it : rb.items) reader.recycle(it);
        sb.t_recycle += now() - tr;
        reader.raw_consumed(rb.items.size());
        return ok;
    };
    // the front of the queue into the index: everything (all), or whatever is ready now -- and more, waiting for the
    // device, while too much is held back behind it
    auto drain = [&](bool all) {
        while (!pending.empty()) {
            Pending &f = *pending.front();
            if (f.batch && !all && raw_in_flight <= gz_in_flight && host_waiting < 4096 &&
                f.run && f.run->ran.wait_for(chrono::seconds(0)) != std::future_status::ready) break;
            const bool ok = f.batch ? append_unit(f) : append_host_run(f);
            pending.pop_front();
            show();
            if (!ok) return false;
        }
        return true;
    };
    const double t_loop = now();
    sb.t_before = t_loop - t_enter;
    for (size_t i = 0; i < files.size(); ++i) {
        const string &fn = files[i];
        const double t0 = now();
        OrderedFastaReader::Item item = reader.take(i);
        sb.t_wait += now() - t0;
        if (item.unit_batch) {
            // a file of a device unit, whatever became of it: the unit stays together, in list order, and runs when its
            // last file has been taken (every file has been put then)
            if (cur && cur->batch != (mk_gz_batch *)item.unit_batch) close_run();
            if (!cur) { cur.reset(new Pending()); cur->batch = (mk_gz_batch *)item.unit_batch; }
            cur->items.push_back(item); cur->names.push_back(fn);
            if (item.unit_last) close_run();
            if (!drain(false)) return;
            continue;
        }
        if (!item.exists) { close_run(); if (!drain(true)) return; sb.log += "Missed file: " + fn + "\n"; show(); reader.recycle(item); continue; }
        if (item.failed) { close_run(); (void)drain(true); if (sb.error.empty()) sb.error = "cannot read " + fn; return; }
        if (item.len < k) { reader.recycle(item); continue; }
        if (cur && cur->batch) close_run();
        if (!cur) cur.reset(new Pending());
        cur->items.push_back(item); cur->names.push_back(fn);
        cur_bytes += item.len;
        if (cur->items.size() >= 64 || cur_bytes > (1ull << 30)) close_run();
        if (!drain(false)) return;
    }
    close_run();
    if (!drain(true)) return;
    sb.t_total = now() - t_loop;
    sb.t_lock = arena_p->lock_s_; sb.slabs = arena_p->n_slabs_;
    // the reader's pool and its page-locked arena are kept until the process ends (~Driver), the inflater's blocks until
    // their context goes: giving gigabytes back takes tenths of a second -- inside the index phase when done here, out of the
    // queries' first batches when done beside them (freeing page-locked or device memory stalls the device) -- and a GPU
    // with 288 GB does not miss them
    {
        std::lock_guard<std::mutex> g(keep_m);
        kept_readers.emplace_back(reader_p.release());
        kept_arenas.push_back(std::move(arena_p));
    }
    if (mk_index_size(ctx) != sb.names.size()) sb.error = string("index build failed: ") + mk_last_error();   // settles the last batch
    sb.t_after = now() - t_loop - sb.t_total;
}

// ---- Miekki.cpp:540-588.  `make_ctx(device ordinal)` creates one shard's context.
void Driver::index_file_of_file(const string &list, const vector<int> &devices, const MakeCtx &make_ctx)
{
    const bool have_list = mkhost::file_exists(list);
    const vector<string> files = have_list ? read_list(list) : vector<string>();
    if (rank_world > 1 || forced_rank_mode) { index_file_of_file_ranked(list, have_list, files, devices, make_ctx); return; }
    // genome shards = contiguous runs of the list, one per GPU (never more shards than files)
    const size_t D = std::max<size_t>(1, std::min<size_t>(devices.size(), files.size()));
    vector<mk_ctx *> ctxs;
    for (size_t d = 0; d < D; ++d) ctxs.push_back(make_ctx(devices[d]));
    group.adopt(ctxs);
    if (!have_list) { cout << "Missed file of file: " << list << endl; finish_index(true); return; }
    vector<ShardBuild> sb(D);
    vector<vector<string>> part(D);
    for (size_t d = 0; d < D; ++d) {
        uint64_t b, e;
        mkhost::shard_range(files.size(), (uint32_t)d, (uint32_t)D, b, e);
        part[d].assign(files.begin() + b, files.begin() + e);
    }
    // reader threads per shard: -t as given for one GPU; with several, -t divided by the shards would leave each
    // with a reader or two (the default -t 8 on 8 GPUs: one), far below what a GPU sketches -- so at least eight
    // per shard, as far as the host's cores go
    // ... the CPUs this process may actually use (affinity mask, cgroup quota -- not hardware_concurrency(), which on a
    // 256-thread host with a 16-CPU quota would start 64 readers for 8 shards); an explicit -t is never exceeded in total
    const unsigned hw = mkhost::usable_cpus();
    const unsigned floor_per = threads_given ? 1u : std::min(8u, std::max(1u, hw / (unsigned)D));
    const unsigned per = D == 1 ? std::max(1u, threads) : std::max(1u, std::max(threads / (unsigned)D, floor_per));
    if (D == 1) {
        build_shard(ctxs[0], part[0], per, true, sb[0]);
    } else {                                                   // the shards build side by side
        vector<std::thread> th;
        for (size_t d = 0; d < D; ++d) th.emplace_back([&, d] { build_shard(ctxs[d], part[d], per, false, sb[d]); });
        for (auto &t : th) t.join();
    }
    for (size_t d = 0; d < D; ++d) {                           // what the reference prints, in list order
        cout << sb[d].log;
        if (!sb[d].error.empty()) { cout << endl << sb[d].error << endl; exit(1); }
        file_names.insert(file_names.end(), sb[d].names.begin(), sb[d].names.end());
    }
    cout << endl;
    if (getenv("MIEKKI_VERBOSE"))
        for (size_t d = 0; d < D; ++d)
            cout << "[ingest] shard " << d << ": " << sb[d].names.size() << " genomes, waited for the readers " << sb[d].t_wait
                 << "s, in mk_index_append " << sb[d].t_append << "s, waited for the device's inflater " << sb[d].t_unpack_wait << "s and for its batches' last kernels " << sb[d].t_free << "s (giving the raw files' buffers back " << sb[d].t_recycle << "s, starting batches " << sb[d].t_start << "s, the whole loop " << sb[d].t_total << "s, before it " << sb[d].t_before << "s, after it " << sb[d].t_after << "s; " << sb[d].slabs << " slabs of 256 MB page-locked, readers waited for them " << sb[d].t_lock << "s); gzip'd files inflated on the device " << sb[d].gz_on_device - sb[d].gz_on_host
                 << ", refused by it and inflated here " << sb[d].gz_on_host << "; sequences that came from the readers " << sb[d].from_readers << endl;
    report_index();
}

// the end of both builds: the shards made one index, and what the reference says of it (Miekki.cpp:583-587)
void Driver::report_index()
{
    finish_index(true);
    compress_cold();
    cout << "Reference indexed: " << group.total() << endl;
    mk_params p;
    mk_get_params(ctx0(), &p);
    if (p.bloom_log2) cout << "BF size:" << int_to_string(1ull << p.bloom_log2) << endl;
}

// rank 0 draws the communicator's id and leaves it where the launcher's other children find it (rendezvous.hpp: a file
// that carries the run's nonce, made exclusively, checked by its readers, gone when everybody has joined)
mk_comm *Driver::make_comm(mk_ctx *ctx)
{
    uint8_t id[MK_COMM_ID_BYTES];
    string err;
    if (rank_id == 0) {
        if (mk_comm_unique_id(id) != MK_OK) die("cannot start RCCL");
        static string to_remove;                                   // (whatever ends this process: the file goes)
        to_remove = meet.path;
        atexit([] { if (!to_remove.empty()) unlink(to_remove.c_str()); });
        if (!mkhost::rendezvous_publish(meet, id, sizeof id, err)) { cout << err << endl; exit(1); }
    } else if (!mkhost::rendezvous_fetch(meet, id, sizeof id, 600000, err)) {   // up to ten minutes: rank 0 may still be starting
        cerr << "rank " << rank_id << ": " << err << endl;
        exit(1);
    }
    mk_comm *comm = nullptr;
    if (mk_comm_create(ctx, rank_id, rank_world, id, &comm) != MK_OK) die("cannot create the communicator");
    if (mk_comm_barrier(comm) != MK_OK) die("communicator barrier failed");
    if (rank_id == 0) mkhost::rendezvous_remove(meet);             // everybody has read it
    return comm;
}

// Every rank says how it fared (empty = well) before the next collective: if any rank failed, ALL leave here, with the
// first failure's words on rank 0's stdout -- nobody is left waiting in a collective the failed rank will never enter.
void Driver::agree(const string &mine, const char *what)
{
    if (!group.ranked()) { if (!mine.empty()) { cout << what << mine << endl; exit(1); } return; }
    vector<string> all;
    string err;
    if (group.all_gather_text(mine, all, err)) { cout << "multi-GPU setup failed: " << err << endl; exit(1); }
    for (const string &e : all)
        if (!e.empty()) { cout << what << e << endl; exit(1); }
}

// ---- one process per GPU (RCCL): this process builds the rank_id-th contiguous run of the list
void Driver::index_file_of_file_ranked(const string &list, bool have_list, const vector<string> &files, const vector<int> &devices,
                                       const MakeCtx &make_ctx)
{
    mk_ctx *ctx = make_ctx(rank_device(devices));
    group.adopt({ctx});
    group.set_comm(make_comm(ctx));
    if (!have_list) { cout << "Missed file of file: " << list << endl; finish_index(true); return; }
    uint64_t b, e;
    mkhost::shard_range(files.size(), (uint32_t)rank_id, (uint32_t)rank_world, b, e);
    const vector<string> part(files.begin() + b, files.begin() + e);
    ShardBuild sb;
    build_shard(ctx, part, std::max(1u, threads), false, sb);
    // what the reference prints while it indexes, and the names of the genomes that were kept: every rank's, in
    // rank order = list order (an error on any rank ends the run on all of them)
    string err, names;
    for (const string &n : sb.names) { names += n; names += '\n'; }
    vector<string> logs, all_names, errors;
    if (group.all_gather_text(sb.error, errors, err) || group.all_gather_text(sb.log, logs, err) ||
        group.all_gather_text(names, all_names, err)) { cout << "multi-GPU setup failed: " << err << endl; exit(1); }
    for (int r = 0; r < rank_world; ++r) {
        cout << logs[r];
        if (!errors[r].empty()) { cout << endl << errors[r] << endl; exit(1); }
        for (const string &n : split_lines(all_names[r]))
            if (!n.empty()) file_names.push_back(n);
    }
    cout << endl;
    report_index();
}

// INDEX->compress_index(1) of main.cpp:198, for the rows that live in host memory (a collection beyond the GPUs' memory):
// packed where related genomes sit next to each other in the list, left alone where nothing is to be gained
void Driver::compress_cold()
{
    for (size_t d = 0; d < group.shards(); ++d) {
        uint64_t raw = 0, packed = 0;
        if (mk_index_compress(group.ctx(d), &raw, &packed) != MK_OK) { cout << "index compression failed: " << mk_last_error() << endl; exit(1); }
        if (raw && getenv("MIEKKI_VERBOSE"))
            cout << "[cold rows] shard " << d << ": " << raw << " bytes in host memory, " << packed << " after packing" << endl;
    }
}

// ---- -M: the genomes of another index file behind the index's own (mk_index_extend): the file is loaded into a second
// context on the same GPU, joined and released.  The joined genomes have no names (an index file stores none).
void Driver::join_index(const string &path, int device)
{
    string err;
    vector<mk_ctx *> src;
    if (mkhost::load_index(path, {device}, src, err, threads) != 0) { cout << "-M: cannot load " << path << ": " << err << endl; exit(1); }
    const uint32_t n = mk_index_size(src[0]);
    const int rc = group.extend(src[0], err);
    mk_destroy(src[0]);
    if (rc != 0) { cout << "-M: joining " << path << " failed: " << err << endl; exit(1); }
    file_names.clear();
    cout << "Genomes joined: " << n << " from " << path << ", the index holds " << group.total() << endl;
}

// ---- -K: the index keeps the genomes `ids` (as -X prints them after -i), in that order (mk_index_select); the file names
// follow, so that output lines and -e, which reads the genomes' files again, stay right
void Driver::keep_genomes(const vector<uint32_t> &ids)
{
    const uint32_t G = group.total();
    for (uint32_t id : ids)
        if (id >= G) { cout << "-K: genome id " << id << " is not in the index (it holds " << G << " genomes)" << endl; exit(1); }
    if (group.shards() > 1 && !std::is_sorted(ids.begin(), ids.end())) {
        cout << "-K: a list that is not in ascending order would move genomes between GPUs: run it on one GPU (MIEKKI_DEVICES=0)" << endl;
        exit(1);
    }
    const bool named = file_names.size() == G;
    string err;
    if (group.select(ids.data(), (uint32_t)ids.size(), err) != 0) { cout << "-K: genome selection failed: " << err << endl; exit(1); }
    if (named) {
        vector<string> kept;
        for (uint32_t id : ids) kept.push_back(file_names[id]);
        file_names.swap(kept);
    }
    cout << "Genomes kept: " << group.total() << endl;
}

// id bases, the global Bloom filter and the sizes of all genomes on the merging GPU
void Driver::finish_index(bool merge_bloom)
{
    string err;
    if (group.finish(merge_bloom, err) != 0) { cout << "multi-GPU setup failed: " << err << endl; exit(1); }
}

}  // namespace mkhost
