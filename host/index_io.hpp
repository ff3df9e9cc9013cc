// Host-side I/O of the `miekki` binary: gzip-transparent text input and the
// on-disk index format of the reference (Miekki.cpp:649-719),
// streamed through the C ABI in partition ranges.  Plain zlib, no HIP.
#pragma once
#include <string>
#include <vector>

#include "miekki_hip.h"
#include "text_file.hpp"                       // file_exists, read_text

namespace mkhost {

// dump_disk: gzip level 1 like zstr::ofstream (zstr.hpp:82), as consecutive 32 MiB
// gzip members compressed by `threads` threads (gzpar.hpp) -- loadable by the
// reference's reader and by zlib's gzread alike.  `ctxs` = the genome shards in id
// order (one context per GPU): their columns side by side are the reference's column.
int dump_index(const std::vector<mk_ctx *> &ctxs, const std::string &path, std::string &err, unsigned threads = 1);
// Miekki(const string&): builds contexts from the file's own header, the genomes split
// in id order over `devices` (never more shards than genomes; every shard receives the
// whole Bloom filter).  Files written by dump_index are inflated by `threads` threads;
// the reference's own dumps (and plain, uncompressed streams) load through gzread.
// slice_world > 0: one process per GPU -- this process is rank slice_rank of slice_world, reads the file like every other
// rank and keeps ONE context (on devices[0]) with the columns of its own run of genomes (the split of the -l build:
// contiguous, in id order), the whole Bloom filter, its genomes' sizes.
// reserve_extra: every context is laid out (mk_reserve) with room for this many genomes more than it loads -- what a join
// (mk_index_extend) is about to add -- so that the matrix is not laid out a second time.
int load_index(const std::string &path, const std::vector<int> &devices, std::vector<mk_ctx *> &out, std::string &err,
               unsigned threads = 1, int slice_rank = -1, int slice_world = 0, uint32_t reserve_extra = 0);
// The 39-byte header of an index file alone (gzip or plain): the parameters a context for it would get (device 0, id base 0)
// and its number of genomes.  false + err: the file cannot be read, is shorter than a header, or is not one this build reads.
bool read_index_header(const std::string &path, mk_params &p, uint32_t &genomes, std::string &err);
// -d with one process per GPU: every rank calls it; the ranks' columns travel to rank 0 a block of rows at a time
// (mk_comm_gather) and rank 0 writes the one stream dump_index would have written from all shards in one process.
// Returns the same value on every rank (err: the first failing rank's words).
int dump_index_ranked(mk_ctx *ctx, mk_comm *comm, const std::string &path, std::string &err, unsigned threads = 1);

}  // namespace mkhost
