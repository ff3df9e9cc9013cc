// `miekki` -- drop-in host driver for the -l / -i / -a / -A / -o / -d / -e command
// line of the reference (main.cpp:125-238) on top of libmiekki_hip.so.
//
// Plain C++ above the C ABI of include/miekki_hip.h: flag parsing, FASTA reading,
// batching, output formatting and the index file format stay on the host exactly
// where the reference has them (file drivers Miekki.cpp:426-645, 723-788); every
// sketch / scan / filter / exact-intersection computation is a call into the HIP
// layer.  Differences from the reference, all deliberate:
//   * genome ids follow list order and output follows query order (what the
//     reference does at -t 1) for every -t; -t sets the number of host threads that
//     read and parse input files ahead of the device,
//   * `-i ... -e` reports that genome file names are not stored in an index
//     instead of crashing,
//   * no zlib re-compression of the in-memory columns (main.cpp:198): they live
//     raw in HBM,
//   * where the reference scales with -t threads inside the one process, this one
//     scales over the visible GPUs inside the one process (MIEKKI_DEVICES=0,1,..
//     restricts them): genome shards in list order, one context per GPU
//     (multi_gpu.hpp); ids, hits and files are those of one GPU,
//   * ... or over one PROCESS per GPU with RCCL between them, when a launcher says so:
//         python -m torch.distributed.run --no-python --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1
//             miekki -l genomes.txt -a queries.fa -o out.txt -h 20        (one command line)
//     (RANK / WORLD_SIZE / LOCAL_RANK from the environment, or MIEKKI_RANK / MIEKKI_WORLD / MIEKKI_LOCAL_RANK): rank r
//     indexes the r-th contiguous run of the list on its own GPU, the Bloom filters are folded by one all-reduce,
//     every rank scans all queries against its shard and ONE ncclGather per batch carries the per-query heap
//     entrants to rank 0, which merges them on its GPU and writes the files and the banners (the other ranks stay
//     silent).  -l with -a / -A (and -e); -i and -d need the single-process form.
//   * the flags that are not in the reference are described where they are implemented: options.hpp holds the rules of
//     all of them, driver_build.cpp -K and -M, driver_query.cpp -X -F -R -r -J -H -O -2 -q, driver_profile.cpp the sinks and -S.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "driver.hpp"
#include "index_io.hpp"
#include "options.hpp"

using namespace std;
using namespace mkhost;

int main(int argc, char **argv)
{
    if (argc < 2) { help(); return 0; }
    // (the HIP runtime folds its streams onto four hardware queues unless told otherwise; the ingest has a dozen streams with
    // work at a time -- a batch's own, the upload streams, the build's -- and a copy that shares a queue with a long kernel of
    // another stream waits behind it: eight queues, unless the user has said something)
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    Options opt;
    parse_options(argc, argv, opt);
    // everything that can be refused is refused here, before a context is made or a file is written (options.hpp)
    Where where;
    const vector<int> devices = device_list();                  // every visible GPU, or MIEKKI_DEVICES
    where.devices = devices.size();
    rank_from_env(where);
    Checked got;
    const string no = refusal(opt, where, got);
    if (got.rank_silenced) cout.setstate(std::ios_base::badbit);              // rank 0 speaks for all
    if (!no.empty()) { cout << no << endl; return 1; }
    const bool rank_mode = where.rank_mode;
    const int rank_id = where.rank_id;
    const unsigned reader_threads = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(opt.core_number, 64));
    const uint32_t bit_per_min = (uint32_t)(5 + opt.fingerprint_size);                              // main.cpp:184
    cout << "Using " << bit_per_min << " bits per minimizer, " << int_to_string(1ull << opt.H) << " minimizers so "
         << int_to_string((uint32_t)(bit_per_min * (1u << opt.H))) << " bits per sequences" << endl;
    auto start = chrono::system_clock::now();
    Driver drv;
    drv.threads = reader_threads;
    drv.threads_given = opt.threads_given;
    drv.nres = opt.nres == 0 ? MK_ALL_RESULTS : (uint32_t)opt.nres;
    drv.mates = opt.mates_file;
    drv.min_qual = opt.qual_given ? (int)opt.min_qual : -1;
    if (rank_mode) {
        drv.rank_id = rank_id; drv.rank_world = where.rank_world; drv.rank_local = where.rank_local; drv.forced_rank_mode = true;
        drv.meet = rendezvous_from_env();
        setenv("MIEKKI_COMM_BANNER_TO_STDERR", "1", 1);              // (stdout is compared with the reference's: mk_comm_create)
    }
    if (!opt.index_file.empty()) {
        if (!file_exists(opt.index_file)) {
            cout << "File problem" << endl;
            return 1;
        }
        string err;
        vector<mk_ctx *> ctxs;
        // -M: the headers of all files first -- a file that is missing or was built with other parameters ends the run before
        // anything is loaded or joined -- and their genomes counted, so that the matrix is laid out once
        uint64_t join_genomes = 0;
        if (!opt.join_files.empty()) {
            mk_params p0, p1;
            uint32_t g0 = 0, g1 = 0;
            if (!read_index_header(opt.index_file, p0, g0, err)) { cout << "Index load failed: " << err << endl; return 1; }
            for (const string &jf : opt.join_files) {
                if (!file_exists(jf)) { cout << "-M: cannot read " << jf << endl; return 1; }
                if (!read_index_header(jf, p1, g1, err)) { cout << "-M: " << err << endl; return 1; }
                const char *differs = p1.k != p0.k ? "-k" : p1.h != p0.h ? "-h" : p1.fp_bits != p0.fp_bits ? "the fingerprint width (-f)"
                                    : p1.bloom_log2 != p0.bloom_log2 ? "-b" : nullptr;
                if (differs) { cout << "-M: " << jf << " and " << opt.index_file << " were built with different parameters: " << differs << " differs" << endl; return 1; }
                join_genomes += g1;
            }
            if (g0 + join_genomes > 0xffffff00ull) { cout << "-M: " << g0 + join_genomes << " genomes are more than an index holds" << endl; return 1; }
        }
        if (rank_mode) {
            // one process per GPU: every rank reads the file and keeps the columns of its run of genomes (main.cpp:189-194,
            // Miekki.cpp:687-719 per rank).  A rank that cannot load still joins the communicator -- on a context of its
            // own making -- so that all ranks hear of it and leave together.
            const int device = drv.rank_device(devices);
            const bool loaded = load_index(opt.index_file, {device}, ctxs, err, reader_threads, rank_id, where.rank_world) == 0;
            if (!loaded) {
                mk_params p{31, 10, 8, 0, 0, device, 0, 0};
                mk_ctx *ctx = nullptr;
                if (mk_create(&p, &ctx) != MK_OK) die("cannot create a context");
                ctxs.assign(1, ctx);
            }
            drv.group.adopt(ctxs);
            drv.group.set_comm(drv.make_comm(ctxs[0]));
            drv.agree(loaded ? string() : (err.empty() ? string("unknown error") : err), "Index load failed: ");
        } else {
            if (load_index(opt.index_file, devices, ctxs, err, reader_threads, -1, 0, (uint32_t)join_genomes) != 0) { cout << "Index load failed: " << err << endl; return 1; }
            drv.group.adopt(ctxs);
        }
        drv.finish_index(false);                            // the file holds the global Bloom filter already
        mk_params p;
        mk_get_params(drv.ctx0(), &p);
        drv.k = p.k; drv.threshold = p.threshold;          // -k -h -f -b -s come from the file (main.cpp:189-194)
        for (const string &jf : opt.join_files) drv.join_index(jf, devices[0]);
        if (!opt.join_files.empty()) drv.compress_cold();       // (a join unpacks cold rows: INDEX->compress_index(1) once, after the last)
        if (!got.keep_ids.empty()) drv.keep_genomes(got.keep_ids);  // (a refused list leaves no output file behind)
        if (!rank_mode || rank_id == 0) drv.out.open(opt.output_file.c_str());
        cout << "I output results in " << opt.output_file << endl;
        cout << "Load sucessful" << endl;
    } else if (!opt.list_file.empty()) {
        if ((!rank_mode || rank_id == 0) && got.keep_ids.empty()) drv.out.open(opt.output_file.c_str());
        cout << "I output results in " << opt.output_file << endl;
        drv.k = (uint32_t)opt.kmer_size; drv.threshold = (uint32_t)opt.threshold;
        drv.index_file_of_file(opt.list_file, devices, [&](int device) {
            mk_params p{(uint32_t)opt.kmer_size, (uint32_t)opt.H, bit_per_min, (uint32_t)opt.bloom_size, (uint32_t)opt.threshold, device, 0, 0};
            mk_ctx *ctx = nullptr;
            const int st = mk_create(&p, &ctx);
            if (st == MK_ERR_UNSUPPORTED) { cout << "not implemented" << endl; exit(0); }          // Miekki.cpp:235-237
            if (st != MK_OK) die("cannot create the index");
            return ctx;
        });
        if (!got.keep_ids.empty()) {
            drv.keep_genomes(got.keep_ids);
            drv.compress_cold();                            // (the selection unpacks cold rows: INDEX->compress_index(1) once more)
            drv.out.open(opt.output_file.c_str());
        }
    } else {
        cout << "What am I supposed to index ? use either -i or -l options please" << endl;
        help();
        return 0;
    }
    if (!opt.families_file.empty()) drv.write_families(opt.families_file);
    if (opt.want_reps()) drv.write_representatives(opt.reps_file, opt.clusters_file);
    if (opt.want_hierarchy()) drv.write_hierarchy(opt.levels_arg, opt.hierarchy_taxonomy_file, opt.hierarchy_order_file);
    if (!opt.index_dump.empty()) {
        cout << "I write this index on the disk for later" << endl;
        string err;
        const int rc = rank_mode ? dump_index_ranked(drv.ctx0(), drv.group.comm(), opt.index_dump, err, reader_threads)
                                 : dump_index(drv.group.contexts(), opt.index_dump, err, reader_threads);
        if (rc != 0) { cout << "Index dump failed: " << err << endl; return 1; }
    }
    auto end_index = chrono::system_clock::now();
    cout << "elapsed time: " << chrono::duration<double>(end_index - start).count() << "s\n";
    if (!opt.query_lines.empty()) {
        if (opt.exact_mode) {
            cout << "running in exact mode, actual intersection will be computed on hits found by the index" << endl;
            drv.query_file_exact(opt.query_lines);
        } else {
            cout << "running in approx mode, intersection is estimated by the index" << endl;
            if (opt.want_profile()) {
                Driver::ProfileJob job;
                job.reads = opt.query_lines;
                job.tally_path = opt.profile_file; job.clade_path = opt.clade_profile_file; job.clades = &got.clade_list;
                job.cover_path = opt.cover_file; job.winners_path = opt.winners_file; job.depth_path = opt.depth_file;
                job.gather_path = opt.gather_file; job.min_new = (uint32_t)opt.min_new;
                job.tax_name = opt.taxonomy_file; job.tax = &got.taxonomy; job.lca_path = opt.lca_report_file; job.nodes_path = opt.lca_reads_file; job.margin = (uint32_t)opt.margin;
                job.taxon_cover_path = opt.taxon_cover_file;
                job.markers_path = opt.markers_file;
                job.abundance_path = opt.abundance_file; job.rounds = (uint32_t)opt.rounds; job.share_margin = (uint32_t)opt.share_margin;
                drv.profile_file(job);
            }
            else drv.query_file(opt.query_lines);
        }
    } else if (opt.index_queries) {
        cout << "running in approx mode, intersection is estimated by the index" << endl;
        drv.query_index();
    } else if (!opt.panel_list.empty()) {
        cout << "running in approx mode, intersection is estimated by the index" << endl;
        drv.panel_files(got.panel_samples, opt.panel_file);
    } else if (!opt.query_list.empty()) {
        if (opt.exact_mode) {
            cout << "running in exact mode, actual intersection will be computed on hits found by the index" << endl;
            drv.query_file_of_file_exact(opt.query_list);
        } else {
            cout << "running in approx mode, intersection is estimated by the index" << endl;
            drv.query_file_of_file(opt.query_list);
        }
    } else {
        cout << "No query file, No queries" << endl;
    }
    auto end_query = chrono::system_clock::now();
    cout << "elapsed time: " << chrono::duration<double>(end_query - end_index).count() << "s\n";
    if (getenv("MIEKKI_VERBOSE") && (drv.group.shards() > 1 || drv.group.ranked()))
        cout << "[exchange] " << (drv.group.ranked() ? (size_t)drv.group.world() : drv.group.shards()) << " shards: " << drv.group.gather_bytes() << " bytes gathered, "
             << drv.group.rerun_queries() << " queries rerun with wide rows, " << drv.group.replayed_queries()
             << " answered from dense score rows" << endl;
    cout << "The end" << endl;
    drv.out.close();
    // One process, its work done and written: leave.  Taking the contexts apart first -- dozens of page-locked pieces, the device's
    // blocks, the streams, one runtime call each -- is 60-80 ms of a run that may be 300 (profiles/r6_cli_startup.txt), for memory
    // the driver takes back anyway when the process ends.  Ranks leave in order: their communicator is shared.
    if (!rank_mode) {
        for (mk_ctx *ctx : drv.group.contexts()) (void)mk_sync(ctx);   // (nothing of the library's is under way, on the device or on a thread)
        cout.flush();
        exit(0);                                             // (not _exit: a profiler's exit handlers write its files)
    }
    return 0;                                                // ~DeviceGroup releases the contexts
}
