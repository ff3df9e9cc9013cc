/* miekki_hip.h -- C ABI of libmiekki_hip.so, the MI355X (gfx950) implementation of
 * Miekki's sketch-build + fingerprint-intersection hot path.
 *
 * The reference has no FFI of its own: main.cpp calls Miekki's members directly.
 * Each entry point below replaces one of those L3 -> L2 calls (citations are into
 * the reference tree) and is what a binding in the
 * reference would bind; INTEGRATION.md shows that binding.
 *
 * Conventions: plain C, opaque handle, every call returns 0 on success or a
 * negative mk_status and leaves a message for mk_last_error() (thread-local).
 * Host pointers unless a parameter name starts with `d_` (device memory of the
 * context's GPU).  One context owns one GPU; calls on one context must not
 * overlap -- with one exception: mk_dev_copy may run with a context as its
 * DESTINATION while another thread uses that context (it reads nothing of the
 * destination but its device ordinal; the multi-GPU driver gathers the shards'
 * rows into the first GPU that way while that GPU still scans).  There is no
 * CPU fallback: without a usable HIP device mk_create fails.
 */
#ifndef MIEKKI_HIP_H
#define MIEKKI_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MK_ABI_VERSION 5

typedef enum {
    MK_OK = 0,
    MK_ERR_ARG = -1,          /* bad argument */
    MK_ERR_UNSUPPORTED = -2,  /* the reference's "not implemented" (Miekki.cpp:235-237, 893-895) */
    MK_ERR_DEVICE = -3,       /* HIP runtime error / no GPU */
    MK_ERR_NOMEM = -4,
    MK_ERR_STATE = -5         /* call not valid in the context's current state */
} mk_status;

typedef struct mk_ctx mk_ctx;

/* Constructor arguments of Miekki(k, h, bit_per_min, 5, 0, out, b, threshold, t)
 * (Miekki.h:66-90, main.cpp:196). */
typedef struct {
    uint32_t k;               /* -k, 2..31 (offsetUpdatekmer = 1 << 2k, Miekki.h:76-77) */
    uint32_t h;               /* -h, log2 of the number of partitions, 1..28 */
    uint32_t fp_bits;         /* number_bit_minimizer = 5 + f: 8 (-f 3) or 16 (-f 11) */
    uint32_t bloom_log2;      /* -b, >= 32 as in the reference */
    uint32_t threshold;       /* -s truncated to u32 (main.cpp:196) */
    int32_t device;           /* HIP device ordinal */
    uint32_t genome_id_base;  /* id of this context's first genome (multi-GPU genome sharding) */
    uint32_t reserved;
} mk_params;

/* Same layout as the reference's similarity_score (Miekki.h:27-31). */
typedef struct {
    uint32_t genome;
    uint32_t matches;
    double jaccard;
    double intersection;
} mk_hit;

/* Device-time accounting of the last query call(s), from HIP events recorded on
 * the context's stream around each kernel. */
typedef struct {
    double sketch_ms;         /* query sketch + Bloom gate */
    double scan_ms;           /* fingerprint scan launches */
    double filter_ms;         /* top-hit selection over the score rows */
    uint64_t scan_launches;
    uint64_t comparisons;     /* G * sum of active partitions */
    uint64_t active_partitions;
    uint64_t scan_algo_bytes; /* comparisons * W + 4 * queries * G */
    double build_sketch_ms;   /* index build: k-mer hashing + minimizer selection */
    double build_finalize_ms; /* transposed matrix write, sizes, Bloom insert */
    uint64_t build_kmers;
    uint64_t build_genomes;
    uint64_t scan_slab_launches; /* of scan_launches: launches of the slab schedule (scan_slab_kernel) */
    /* mk_dev_copy calls with this context as the SOURCE, by the path they took: a direct GPU-to-GPU
     * copy (same GPU, or peer access over xGMI), or through host memory because the two GPUs have
     * no peer access -- a staged exchange would otherwise just look like a slow xGMI */
    uint64_t peer_copies, staged_copies;
    uint64_t peer_copy_bytes, staged_copy_bytes;
} mk_stats;

const char *mk_last_error(void);
uint32_t mk_abi_version(void);

/* new Miekki(...)  (main.cpp:196) */
int mk_create(const mk_params *params, mk_ctx **out);
void mk_destroy(mk_ctx *ctx);

/* Pre-size the fingerprint matrix for n_genomes rows per partition.  Optional;
 * appending past the reservation re-lays the matrix out (needs 2x memory).
 * A matrix larger than its HBM budget (environment MIEKKI_HBM_MATRIX_MIB, or simply
 * more than the free device memory) keeps its first partition rows in HBM and the rest
 * in page-locked host memory; every entry point works unchanged, queries over the cold
 * partition ranges are streamed at PCIe speed.  (What compress_index / decompress_index,
 * Miekki.cpp:863-877, were for in the reference: a collection beyond fast memory.) */
int mk_reserve(mk_ctx *ctx, uint32_t n_genomes);

/* Miekki::compress_index / decompress_index (Miekki.cpp:863-877; main.cpp:198 compresses after -l) for the rows that live
 * in host memory because the matrix exceeds its HBM budget (mk_reserve): per piece of 1,024 genomes of a row, one bit per
 * genome "differs from the genome before" + the differing fingerprints -- what related strains next to each other in the
 * list leave of a column (README.md:136-138); a row that would not shrink is kept as it is, and a collection that does
 * not shrink by 5 % is left alone.  Queries then move the PACKED bytes of a cold range over PCIe and expand them in HBM;
 * appends, exports and imports unpack first by themselves (the reference's dump decompresses first too, 662-664).
 * raw_bytes / packed_bytes (may be NULL): the cold rows before and after (equal: nothing was packed). */
int mk_index_compress(mk_ctx *ctx, uint64_t *raw_bytes, uint64_t *packed_bytes);
int mk_index_decompress(mk_ctx *ctx);
uint32_t mk_index_size(const mk_ctx *ctx);                 /* Miekki::index_size */
int mk_get_params(const mk_ctx *ctx, mk_params *out);
int mk_get_stats(const mk_ctx *ctx, mk_stats *out);
int mk_reset_stats(mk_ctx *ctx);
/* Measurement aid (bench.py): best of `rounds` read-only streaming passes (16-byte loads,
 * eight in flight per lane) over the resident fingerprint matrix -> GB/s and the bytes one
 * pass read.  The box's own HBM read ceiling, to put beside the 8 TB/s spec figure. */
int mk_probe_stream_read(mk_ctx *ctx, uint32_t rounds, double *gbps, uint64_t *bytes);
/* Measurement aid (bench.py's PCIe-fed build sample): the synthetic genomes of SURVEY.md 8d
 * (ids first_id .., `length` bases each, concatenated) written to host memory dst. */
int mk_probe_synth_genomes(mk_ctx *ctx, uint64_t first_id, uint32_t n, uint64_t length, char *dst);
/* Test aid: the query-block scan's compare alone.  flags[i] = for every byte (width 1) or half-word (width 2) of the
 * word d[i], 1 in its lowest bit where it differs from that of b[i], 0 where it is equal.  Host arrays of n words. */
int mk_probe_ne_lanes(mk_ctx *ctx, uint32_t width, const uint32_t *d, const uint32_t *b, uint64_t n, uint32_t *flags);

/* ---- index build --------------------------------------------------------- */

/* Miekki::insert_sequences (Miekki.cpp:277-314; called from index_file_of_file,
 * Miekki.cpp:572,580).  Genome ids follow call order.  Sequences shorter than k
 * are rejected with MK_ERR_ARG (the driver filters them, Miekki.cpp:569).
 * Pipelined: the sequences are copied to the GPU while the kernels of the previous
 * call still run; the call returns when the copy is done (seqs may be reused) and
 * leaves this batch's kernels in flight.  Every other entry point first settles
 * the batch in flight, so results are always those of a synchronous build. */
int mk_index_append(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t n);

/* Miekki::insert_sequence (Miekki.cpp:243-273; behind index_file, 518-536 -- neither is reached from the reference's
 * CLI, both are public members).  One genome; sketch, column and Bloom inserts are insert_sequences', the size estimate
 * is this member's own: the count of active partitions is a double there, so its square does not wrap at 2^32 the way
 * insert_sequences' u32 does (Miekki.cpp:289, 306) -- genome_size differs from mk_index_append's above 65,535 active
 * partitions, i.e. from -h 17 on. */
int mk_index_insert_sequence(mk_ctx *ctx, const char *seq, uint64_t len);

/* ---- packed ingest (2-bit packing overlapped with the copy to the GPU) ----
 * A sequence as 2 bits per base and, only when it holds characters other than A, C, G, T, one
 * exception bit per base -- a quarter (three eighths) of the bytes mk_index_append moves:
 *   codes   base i at bits 2 * (i % 32) of 64-bit word i / 32: A 0, C 1, G 2, T 3, anything else 0
 *           (nuc2int, utils.cpp:31-49)
 *   except  bit i % 64 of word i / 64 is set where the character is not one of "ACGT" (upper case):
 *           for those the reverse strand's digit is 0 as well, not 3 - code (nuc2intrc,
 *           utils.cpp:107-125); NULL when the sequence has none
 *   head    the first min(len, 32) characters as they came: the k-1 characters of the seed go
 *           through str2numstrand (utils.cpp:252-272: case-insensitive, any other character zeroes
 *           the whole seed), which codes and exception bits cannot express
 * Results are those of mk_index_append on the characters, bit for bit. */
typedef struct {
    const uint64_t *codes;    /* (len + 31) / 32 words */
    const uint64_t *except;   /* (len + 63) / 64 words, or NULL */
    uint64_t len;             /* bases */
    char head[32];
} mk_packed_seq;

/* Host-side packer (no GPU involved; thread-safe, AVX2 when the CPU has it): appends n characters at
 * base position `at` of a sequence being packed, e.g. FASTA line by FASTA line straight into
 * page-locked buffers (mk_host_alloc).  The words that hold position `at` keep their lower positions,
 * everything above at + n in the words written becomes zero: pack in ascending order, nothing needs
 * clearing first.  Both arrays must have room for mk_pack_code_words / mk_pack_except_words of the
 * final length.  Returns 1 when any of the n characters was an exception (hand `except` over then),
 * 0 when none was, -1 on a null argument. */
uint64_t mk_pack_code_words(uint64_t len);
uint64_t mk_pack_except_words(uint64_t len);
int mk_pack_append(uint64_t *codes, uint64_t *except, uint64_t at, const char *chars, uint64_t n);

/* Miekki::insert_sequences (Miekki.cpp:277-314) for packed sequences; pipelined like
 * mk_index_append (the arrays may be reused when the call returns). */
int mk_index_append_packed(mk_ctx *ctx, const mk_packed_seq *seqs, uint32_t n);

/* Page-locked host memory for sequences handed to mk_index_append / mk_qset_upload:
 * from such buffers the copy to the GPU is a direct DMA (no staging copy on the
 * host) and runs beside the kernels.  Ordinary memory works too, only slower.
 * Thread-safe. */
int mk_host_alloc(mk_ctx *ctx, uint64_t bytes, void **out);
void mk_host_free(mk_ctx *ctx, void *p);

/* mk_index_append for the synthetic genomes of SURVEY.md 8d, generated on the device
 * (ids first_id .. first_id+n-1, `length` bases each): no PCIe traffic. */
int mk_index_append_synthetic(mk_ctx *ctx, uint64_t first_id, uint32_t n, uint64_t length);
/* The same for a collection of RELATED genomes (measurement aid for the column codec, mk_index_compress): genome g is
 * strain g % strains of species g / strains; strain 0 is the synthetic genome `species` of SURVEY.md 8d itself, the
 * others are independent descendants of it with about rate_ppm substitutions per million bases (tests/synth.py:
 * strain_device is the same generator on the host). */
int mk_index_append_synthetic_strains(mk_ctx *ctx, uint64_t first_id, uint32_t n, uint64_t length, uint32_t strains,
                                      uint32_t rate_ppm);

/* ---- gzip'd input on the device.  The reference reads every genome file through zstr::ifstream (Miekki.cpp:559-567;
 * zstr.hpp:78: inflateInit2(15 + 32), i.e. gzip members or plain text); these calls take the FILES' bytes as they are.
 * A file is decoded only if it is nothing but well-formed gzip members from its first byte to its last, every member's
 * CRC-32 and ISIZE included; anything else gets a status and is left to the caller's own inflater. */
typedef enum {
    MK_GZ_OK = 0,
    MK_GZ_EMPTY = 1,          /* no stream */
    MK_GZ_NOT_GZIP = 2,       /* no gzip header where one must be (magic, method, reserved flags) */
    MK_GZ_TRUNCATED = 3,      /* the input ends inside a member */
    MK_GZ_BAD_BLOCK = 4,      /* block type 3 */
    MK_GZ_BAD_STORED = 5,     /* a stored block's length and its complement disagree */
    MK_GZ_BAD_LENGTHS = 6,    /* a block's code lengths: over-subscribed, incomplete, bad repeat, no end-of-block code */
    MK_GZ_BAD_CODE = 7,       /* bits that are no code of the block's code */
    MK_GZ_BAD_DISTANCE = 8,   /* a match that reaches back beyond the member's first byte */
    MK_GZ_TOKEN_ROOM = 9,     /* (no longer reported: segments that outgrow their token slots are decoded again with exact rooms) */
    MK_GZ_OUTPUT_ROOM = 10,   /* more text than the room given */
    MK_GZ_TRAILING = 11,      /* bytes behind the last member that are not another member */
    MK_GZ_BAD_CRC = 12,
    MK_GZ_BAD_SIZE = 13,
    MK_GZ_INTERNAL = 14       /* the decoder disagrees with itself (never expected; the file goes to the host like any other failure) */
} mk_gz_status;

/* n whole files -> their text in out[i] (room out_room[i] bytes): out_bytes[i] and status[i] (mk_gz_status) per file. */
int mk_gz_inflate(mk_ctx *ctx, const uint8_t *const *gz, const uint64_t *gz_bytes, uint32_t n, uint8_t *const *out,
                  const uint64_t *out_room, uint64_t *out_bytes, int32_t *status);

/* n genome FILES (gzip'd FASTA) inflated and kept as text ON THE DEVICE, their sequences as index_file_of_file reads them
 * (Miekki.cpp:559-567: every line that does not start with '>' appended, line feeds dropped) measured: mk_gz_sequence says
 * how long file i's is, mk_index_append_gz appends files of the batch -- their sequences are stripped out of the text straight
 * into the build's buffers, nothing crosses PCIe again.  A file whose status is not MK_GZ_OK has no sequence here: inflate it
 * on the host.  The batch's memory (the files, their text and about as much again) is the context's until mk_gz_free -- the
 * appends that read it must have returned -- and stays with the context for the next batch until mk_gz_trim or mk_destroy.
 * mk_gz_unpack works on a stream of its own and touches nothing of the context but its device and its list of spare memory:
 * it may run on a thread of its own while other calls use the context (the driver inflates the next batch while it appends
 * the one before). */
typedef struct mk_gz_batch mk_gz_batch;
int mk_gz_unpack(mk_ctx *ctx, const uint8_t *const *gz, const uint64_t *gz_bytes, uint32_t n, mk_gz_batch **out);
/* mk_gz_unpack in steps, for a caller whose reader threads fetch the files themselves (zstr's read loop, zstr.hpp:186-190, is
 * what they replace): mk_gz_open lays the batch out from the files' sizes; mk_gz_put hands over bytes [at, at + bytes) of file i
 * -- staged != 0: `data` is a page-locked piece lent by mk_gz_stage (*cap bytes; NULL when none is to be had), the copy is a
 * DMA nobody waits for and the piece is the library's again; staged == 0: any memory, copied before the call returns --;
 * mk_gz_run, when every file has been put, inflates and measures the sequences (mk_gz_sequence, mk_index_append_gz).  mk_gz_stage
 * and mk_gz_put may be called from any number of threads at once; a file never put reads as empty (MK_GZ_NOT_GZIP). */
int mk_gz_open(mk_ctx *ctx, const uint64_t *gz_bytes, uint32_t n, mk_gz_batch **out);
void *mk_gz_stage(mk_gz_batch *batch, uint64_t *cap);
int mk_gz_put(mk_gz_batch *batch, uint32_t i, uint64_t at, const void *data, uint64_t bytes, int staged);
/* the files' places in the batch's input: offsets[0 .. n] (file i's bytes at offsets[i], zeros from its end to offsets[i + 1]);
 * files that follow each other, laid out like that in one piece, go with one call (and one copy): mk_gz_put_span */
int mk_gz_layout(const mk_gz_batch *batch, uint64_t *offsets);
int mk_gz_put_span(mk_gz_batch *batch, uint32_t first, uint32_t count, const void *data, uint64_t bytes, int staged);
int mk_gz_run(mk_gz_batch *batch);
int mk_gz_sequence(const mk_gz_batch *batch, uint32_t i, uint64_t *len, int32_t *status);
/* insert_sequences (Miekki.cpp:277-314) for files which[0 .. n) of the batch, in that order (each must have status MK_GZ_OK and
 * at least k characters); pipelined like mk_index_append. */
int mk_index_append_gz(mk_ctx *ctx, const mk_gz_batch *batch, const uint32_t *which, uint32_t n);
void mk_gz_free(mk_gz_batch *batch);
void mk_gz_trim(mk_ctx *ctx);                /* give the device memory kept between batches back (after a build) */

/* ---- persistence: the payload of dump_disk / the loading constructor
 * (Miekki.cpp:649-719), streamed in ranges so that the host never
 * needs the whole matrix at once. --------------------------------------------- */

/* columns [p_begin, p_end): (p_end-p_begin) * G * (fp_bits/8) bytes, partition-
 * major, 16-bit values big-endian -- byte-for-byte what dump_disk writes. */
int mk_index_export_columns(mk_ctx *ctx, uint32_t p_begin, uint32_t p_end, uint8_t *dst);
/* The columns of n chosen genomes (ids as the context reports them), every partition: dst[p][j] = the
 * fingerprint of genome ids[j] in partition p, 2^h * n * (fp_bits/8) bytes in dump_disk's byte order --
 * what dump_disk (Miekki.cpp:665-668) would write as the column block of an index holding just those genomes.
 * A sample of a 100,000-genome collection costs megabytes this way, not an export of the whole matrix. */
int mk_index_export_genomes(mk_ctx *ctx, const uint32_t *ids, uint32_t n, uint8_t *dst);
/* mk_index_export_genomes with the block left on the device (d_dst: 2^h * n * W bytes) */
int mk_index_export_genomes_device(mk_ctx *ctx, const uint32_t *ids, uint32_t n, uint8_t *d_dst);
int mk_index_export_sizes(mk_ctx *ctx, uint64_t *genome_size, uint32_t *sketch_size);
/* Bloom bytes [begin, end) of the 2^(b-3)-byte table */
int mk_index_export_bloom(mk_ctx *ctx, uint64_t begin, uint64_t end, uint8_t *dst);

int mk_index_import_begin(mk_ctx *ctx, uint32_t n_genomes);    /* empties the index first */
int mk_index_import_columns(mk_ctx *ctx, uint32_t p_begin, uint32_t p_end, const uint8_t *src);

/* mk_index_import_columns for rows that are still Huffman-coded -- the form this program's own index files keep the
 * fingerprint columns in (host/fastz.cpp, deflate_huffman_only: deflate blocks of literals only, one Huffman code of at
 * most 12 bits per MiB, a block per 16 KiB; each gzip member's extra field lists where every block's first symbol lies).
 * The device inflates them, one lane per block (huff.hip): the reference's `in->read` of the columns (Miekki.cpp:708-712)
 * without an inflater on the host.  `payload`: the members' deflate streams as they lie in the file, one after the other
 * (page-locked memory makes the copy a DMA).  `blocks`: n_blocks of them, a multiple of 64 -- every 64 consecutive entries
 * use ONE code (entry 64 i's `code`; slots with out_len 0 fill a group up) -- that together produce exactly the bytes of
 * rows [p_begin, p_end) in the dump's byte order.  `lens`: n_codes x 257 code lengths (literals 0 .. 255, end-of-block).
 * Out: crc_out[i] = the CRC-32 remainder of block i's bytes (start value 0, no final complement: the caller folds them
 * with the blocks' lengths and compares with the members' trailers); *bad_out = blocks whose code is not a complete code
 * of at most 12 bits, that point outside the payload or the rows, hold an end-of-block code early or lack it at their
 * end -- the index is not usable unless it is 0 and the CRCs hold. */
typedef struct {
    uint64_t bit;       /* where the block's first symbol starts: bits from payload[0] */
    uint64_t out;       /* where its bytes go: bytes from the first byte of row p_begin */
    uint32_t out_len;   /* how many bytes it holds */
    uint32_t code;      /* which of the n_codes length tables it is coded with */
} mk_huff_block;
int mk_index_import_columns_huffman(mk_ctx *ctx, uint32_t p_begin, uint32_t p_end, const uint8_t *payload, uint64_t payload_bytes,
                                    const mk_huff_block *blocks, uint32_t n_blocks, const uint8_t *lens, uint32_t n_codes,
                                    uint32_t *crc_out, uint32_t *bad_out);
int mk_index_import_sizes(mk_ctx *ctx, const uint64_t *genome_size, const uint32_t *sketch_size);
int mk_index_import_bloom(mk_ctx *ctx, uint64_t begin, uint64_t end, const uint8_t *src);

/* Keep the n genomes ids[0 .. n) of the index, in that order, in place: afterwards the index holds n genomes and genome
 * j is the genome that was ids[j] -- drop genomes, cut a sub-index, put related genomes next to each other (what
 * mk_index_compress gains from).  The reference has no such member; the result is DEFINED by the stream of
 * dump_disk / the loading constructor (Miekki.cpp:649-719): the index is what the reference holds after loading a file
 * with index_size = n, the columns old_column[ids[j]] in every partition, genome_size[ids[j]], the Bloom filter AS IT
 * WAS and sketch_size[ids[j]], bit for bit.  The filter is not touched: cells cannot be un-inserted and a cell's byte
 * belongs to its first writer, so the result is not always a fresh build of the kept genomes -- a partition of a query
 * whose k-mer only a removed genome held stays active; it matches nothing but counts in `active`.
 * ids as the context reports them (genome_id_base stays), distinct: n == 0, a null list, an id outside the index or an
 * id named twice is MK_ERR_ARG and leaves the index exactly as it was (all checked on the host before any launch); the
 * current order is valid and changes nothing.  A build batch in flight is settled first, packed cold rows are unpacked
 * first (as the exports do) and stay unpacked.  Capacity, pitch and the placement of the rows (HBM / host) do not
 * change and no memory is given back (dump and reload for a smaller footprint); columns [n, old size) of every row are
 * zero afterwards, as a later append expects.  The rows are gathered on the device through the column staging buffer
 * (keep.hip) and never cross PCIe, other than cold rows, which stay where they are.
 * Query sets: uploaded sequences re-sketch, sets made by mk_qset_from_columns keep their own copy; a set made by
 * mk_qset_from_index BEFORE the call names genomes by ids that now mean other genomes and fails its next run, scores or
 * list call with MK_ERR_STATE (so does one made before mk_index_import_begin). */
int mk_index_select(mk_ctx *ctx, const uint32_t *ids, uint32_t n);

/* Join two indexes: src's genomes are appended behind dst's, in src's order -- local genome j of src becomes local genome
 * G_dst + j of dst; dst's genome_id_base and threshold stay, src keeps its content and stays usable.  The reference only
 * has an unfinished member for this (Miekki::merge_indexes, Miekki.cpp:901-910: it forgets both size arrays and the
 * filter), so the result is DEFINED by the build: afterwards dst is the index the reference holds after insert_sequences
 * of dst's genomes followed by src's, bit for bit -- columns, genome_size, sketch_size and the Bloom filter.  That is
 * exact: a genome's column and sizes depend on its own sequence only (Miekki.cpp:277-314), and a Bloom cell keeps the
 * byte of its first writer in genome order (Miekki.cpp:121-131), so the joint filter is dst's byte where that is non-zero
 * and src's byte otherwise.  A later append on dst is still a joint build.
 * Refused on the host before anything changes: a null argument, dst == src, k, h, fp_bits or bloom_log2 that differ (the
 * message names the first that does), more genomes than an index holds or ids beyond 32 bits: MK_ERR_ARG; contexts on
 * different devices: MK_ERR_UNSUPPORTED.  An empty src: MK_OK, nothing changes; an empty dst becomes src's content under
 * its own header.  Build batches in flight on either context are settled first, packed cold rows on either are unpacked
 * first (as the exports do) and stay unpacked.  dst grows as for an append (a dst reserved for the total with mk_reserve
 * is not laid out again); rows of either index beyond its HBM budget stay in host memory and are read / written there.
 * Both indexes have to be resident: there is no streaming of a file into place.  The columns move on the device
 * (extend.hip), the sizes device to device.
 * Query sets: the ids of dst's genomes mean what they meant, so a set made by mk_qset_from_index before the call runs
 * again afterwards (re-gathered, as after an append) and sees the new genomes. */
int mk_index_extend(mk_ctx *dst, mk_ctx *src);

/* ---- queries --------------------------------------------------------------- */

/* Miekki::query_sequences (Miekki.cpp:344-372): scores[nq][G], row-major u32. */
int mk_query_scores(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq,
                    uint32_t *scores);

/* filter_results(query_sequences(batch), nresults, min_score, min_intersection)
 * (Miekki.cpp:437; 376-422): hits[nq][nresults], nhits[nq]; each row descending by
 * intersection with the reference's heap tie behaviour.  active[nq] (may be NULL)
 * receives query_sequence's active_minimizer (Miekki.cpp:318-340). */
int mk_query(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq,
             uint32_t nresults, uint32_t min_score, double min_intersection,
             mk_hit *hits, uint32_t *nhits, uint32_t *active);

/* filter_results(query_sequences(batch), nresults, ...) (Miekki.cpp:437, 500; 376-397) for ANY nresults, on the device
 * for the whole batch: the reference's driver hard-codes ten; "the list of genomes that share more than S k-mers" is
 * nresults = index_size, spelled MK_ALL_RESULTS here.  The result is a CSR list owned by the library: offsets[nq + 1]
 * into hits, each query's hits exactly what filter_results returns for that nresults -- descending intersection, equal
 * intersections in the order libstdc++'s push_heap / pop_heap / sort_heap leave them in.  mk_query's answer for
 * nresults <= 64 is the same list.  nresults = MK_LIST_CANDIDATES skips the heap: every genome that passes min_score and
 * min_intersection (381-384) in ascending genome id -- what the shards of a sharded index hand to mk_filter_candidates,
 * concatenated in shard order.  active[nq] (may be NULL) as in mk_query.  Free the list with mk_hitlist_free. */
#define MK_ALL_RESULTS 0xffffffffu
#define MK_LIST_CANDIDATES 0xfffffffeu
typedef struct mk_hitlist mk_hitlist;
int mk_query_list(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t nresults,
                  uint32_t min_score, double min_intersection, mk_hitlist **out, uint32_t *active);
const uint64_t *mk_hitlist_offsets(const mk_hitlist *list);      /* nq + 1 */
const mk_hit *mk_hitlist_hits(const mk_hitlist *list);           /* offsets[nq] records */
void mk_hitlist_free(mk_hitlist *list);

/* Pure host function: the heap of Miekki::filter_results (Miekki.cpp:386-396) over
 * candidates that already passed both thresholds, given in ascending genome
 * order (all of them, or just the heap entrants mk_qset_run emits).  Used by
 * mk_query and by the multi-GPU merge on rank 0. */
uint32_t mk_filter_candidates(const mk_hit *cand, uint32_t ncand, uint32_t nresults, mk_hit *out);

/* The same heap on the device, for whole batches: d_count[world][nq] and
 * d_cand[world][nq][cap] are the entrant rows of `world` genome shards in shard
 * order (world = 1: what mk_qset_run wrote; world > 1: the gathered rows on rank
 * 0).  Writes d_hits[nq][nresults] and d_nhits[nq]; a query for which some shard's
 * count exceeds `cap` gets d_nhits = MK_MERGE_OVERFLOW and no hits (answer it
 * again from a dense score row).  nresults <= 64.  All pointers are device
 * memory; asynchronous on the context's stream. */
#define MK_MERGE_OVERFLOW 0xffffffffu
int mk_merge_entrants(mk_ctx *ctx, const uint32_t *d_count, const mk_hit *d_cand, uint32_t world,
                      uint32_t nq, uint32_t cap, uint32_t nresults, mk_hit *d_hits, uint32_t *d_nhits);

/* filter_results' heap over gathered exchange rows: d_rows[world][nq][1 + cap] (what
 * mk_qset_run_compact wrote on `world` genome shards, in shard order).  Sizes of the
 * genomes the rows name come from mk_merge_set_sizes (all shards' sketch_size /
 * genome_size concatenated in shard order; id_base = id of entry 0); without it, and
 * with world == 1, the context's own index is used.  Output as mk_merge_entrants. */
int mk_merge_set_sizes(mk_ctx *ctx, const uint64_t *genome_size, const uint32_t *sketch_size,
                       uint32_t n_genomes, uint32_t id_base);
/* the sizes mk_merge_set_sizes (or mk_comm_share_sizes) left on the context, back on the host (n = how many were set) */
int mk_merge_get_sizes(mk_ctx *ctx, uint64_t *genome_size, uint32_t *sketch_size, uint32_t n);
int mk_merge_compact(mk_ctx *ctx, const uint64_t *d_rows, uint32_t world, uint32_t nq, uint32_t cap,
                     uint32_t nresults, mk_hit *d_hits, uint32_t *d_nhits);

/* ---- device-resident query sets (bench / multi-GPU path) ------------------- */

typedef struct mk_qset mk_qset;

/* Upload sequences once; they stay in HBM until mk_qset_free. */
int mk_qset_upload(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq,
                   mk_qset **out);
/* Read pairs: query q of the set is the PAIR (seqs1[q], seqs2[q]), one query, not two.  Its k-mers are those
 * minhash_sketch_partition (Miekki.cpp:150-197) walks in mate 1 alone and those it walks in mate 2 alone: each mate has its
 * own k-1 seed by str2numstrand's rules and its own skipped last k-mer, and no k-mer spans the junction.  Per partition the
 * smallest fingerprint wins, the k-mer met first among equals, mate 1 before mate 2 (the reference's strict `<`): with
 * (fa, ha) and (fb, hb) the fingerprints and hashes of the two mates' sketches, mate 2 takes partition p where
 * fb[p] < fa[p], with ITS hash.  The Bloom gate of minhash_sketch_partition_solid_kmers (Miekki.cpp:214-224, check_bloom
 * 135-146) is then asked for the winner's hash: a winner it drops leaves the partition empty -- the loser does not step in.
 * So a pair's gated sketch is neither the union of its mates' gated sketches nor the sketch of the two joined into one
 * sequence.  (a, ""), ("", a) and (a, a) are the read a; a mate of at most k characters adds nothing; the k-mers are
 * canonical, so the mates' orientation needs no flag.  Scores, mk_qset_active and every sink follow from the gated sketch
 * as for a single sequence: the result is an ordinary set for every mk_qset_* call, sketched again as pairs after
 * mk_qset_invalidate and whenever the index has changed.  A null array with nq > 0: MK_ERR_ARG.  A pair with more than
 * 4,096 k-mers in all: MK_ERR_UNSUPPORTED, the message names its index (paired reads are short reads). */
int mk_qset_upload_pairs(mk_ctx *ctx, const char *const *seqs1, const uint64_t *lens1, const char *const *seqs2,
                         const uint64_t *lens2, uint32_t nq, mk_qset **out);
/* Reads with base qualities: query q is the sequence seqs1[q] of lens1[q] characters with the quality string quals1[q] of the
 * same length, Sanger / Illumina 1.8+ coding (phred + 33).  Base j is GOOD when (uint8_t)quals1[q][j] >= 33 + min_qual --
 * quality alone decides; an N or a lower-case letter is whatever the reference makes of it.  The read's SEGMENTS are its
 * maximal runs of good bases, in order; a bad base belongs to no segment.  Each segment is a sequence of its own for
 * minhash_sketch_partition (Miekki.cpp:150-197): its own k-1 seed by str2numstrand's rules (case-insensitive inside the
 * seed, one invalid character zeroes the whole seed) and its own skipped last k-mer, so the k-mer at window start i exists
 * exactly when the k + 1 bases [i, i + k] are inside the read and all good.  The read is ONE query: per partition the smallest
 * fingerprint over all segments wins, the k-mer met first among equals -- the earliest segment, by the reference's strict
 * `<` -- with ITS hash, and the Bloom gate of minhash_sketch_partition_solid_kmers (Miekki.cpp:214-224, check_bloom 135-146)
 * is asked for that winner alone: a winner it drops leaves the partition empty.  This is mk_qset_upload_pairs' rule folded
 * over n pieces instead of two, the cuts found on the device.  With min_qual = 0 every base is good: the read is the plain
 * read.  A read with one bad base at c is the pair (s[:c], s[c+1:]).
 * seqs2, lens2 and quals2 are all null for single reads and all non-null for PAIRS WITH QUALITIES: the same fold over the
 * segments of mate 1, then those of mate 2; the junction between the mates is a cut that consumes no base.
 * The result is an ordinary set for every mk_qset_* call, sketched again under the same rule after mk_qset_invalidate and
 * whenever the index has changed.  MK_ERR_ARG: a null array with nq > 0, mate-2 arrays only partly given, min_qual > 93.
 * MK_ERR_UNSUPPORTED, the message names the index: a read or pair of more than 4,096 characters in all (these are short
 * reads; longer queries do not learn about qualities). */
int mk_qset_upload_reads(mk_ctx *ctx, const char *const *seqs1, const uint64_t *lens1, const char *const *quals1,
                         const char *const *seqs2, const uint64_t *lens2, const char *const *quals2,
                         uint32_t nq, uint32_t min_qual, mk_qset **out);
/* SURVEY 8d synthetic queries first_id.. cut from synthetic genomes
 * (id mod n_genomes_total, length genome_len), generated on the device. */
int mk_qset_synthetic(mk_ctx *ctx, uint64_t first_id, uint32_t nq, uint64_t n_genomes_total,
                      uint64_t genome_len, uint64_t query_len, mk_qset **out);
/* query_sequence(sequence of genome ids[j]) without the sequence: the genome's stored column IS its gated sketch
 * (Miekki.cpp:281/320 same sketch; 295-299 + 135-146: the gate passes every active partition of an indexed genome).
 * ids as the context reports them, in any order, repeats allowed; an id outside the index or n == 0: MK_ERR_ARG.  An
 * ordinary set of whole-genome queries for every mk_qset_* call: mk_qset_active = sketch_size[ids[j]], mk_stats.sketch_ms
 * carries the gather.  The columns are gathered again whenever the index has changed (genomes appended: the rows grow);
 * a set made before the ids changed their meaning (mk_index_import_begin, mk_index_select) fails its next run with MK_ERR_STATE.  Runs of 64
 * consecutive ids are gathered with 16-byte loads, anything else byte by byte.  A packed index (mk_index_compress) is
 * unpacked first, as the exports do. */
int mk_qset_from_index(mk_ctx *ctx, const uint32_t *ids, uint32_t n, mk_qset **out);
/* the same from columns the caller holds on the context's GPU: d_cols[2^h][n], dump_disk byte order (what
 * mk_index_export_genomes produces) -- for the shards of a sharded index that do not own the genomes.  The set keeps its
 * own copy (d_cols may go when the call returns) and never gathers again. */
int mk_qset_from_columns(mk_ctx *ctx, const uint8_t *d_cols, uint32_t n, mk_qset **out);
void mk_qset_free(mk_ctx *ctx, mk_qset *qs);

/* One pass of the hot path over the set: sketch + Bloom gate + scan + top-hit
 * selection.  For every query the device emits, in ascending genome id, the
 * ENTRANTS of filter_results' heap (Miekki.cpp:376-397): the genomes that pass
 * min_score / min_intersection and are not skipped by the heap-minimum test
 * (Miekki.cpp:387) for a heap of `nresults` (<= 64).  Only entrants shape the
 * reference's result, so mk_filter_candidates over a row reproduces it exactly;
 * rows of several genome shards concatenated in shard order do too (multi-GPU
 * merge).  Output goes to device memory owned by the caller: d_count[nq] (u32; a
 * value above `cap` marks a row that overflowed) and d_cand[nq][cap] (mk_hit).
 * Asynchronous on the context's stream; mk_sync waits.
 * min_score 0 over an index that holds a genome with sketch_size 0 (a sequence
 * exactly k long) would make NaN intersections (0 / 0, Miekki.cpp:381-383), whose
 * fate in the reference's heap follows no order: MK_ERR_UNSUPPORTED -- mk_query
 * answers such calls, through the host's own heap calls. */
int mk_qset_run(mk_ctx *ctx, mk_qset *qs, uint32_t nresults, uint32_t min_score,
                double min_intersection, uint32_t cap, uint32_t *d_count, mk_hit *d_cand);
/* The same pass with the output in the 8-byte EXCHANGE form of the multi-GPU path
 * ("(genome_id u32, score u32)" per entrant): d_rows[nq][1 + cap] 64-bit
 * words per query -- word 0 = number of entrants (a value above `cap` marks a row that
 * overflowed), then genome | matches << 32 in ascending genome id.  jaccard and
 * intersection are not shipped: the merging side recomputes them from the two sizes
 * of the genome (mk_merge_set_sizes) with the reference's operations
 * (Miekki.cpp:382-383), bit-identically.  One buffer, so one collective. */
int mk_qset_run_compact(mk_ctx *ctx, mk_qset *qs, uint32_t nresults, uint32_t min_score,
                        double min_intersection, uint32_t cap, uint64_t *d_rows);
/* mk_query_list over a prepared set (Miekki.cpp:437 with any nresults, MK_ALL_RESULTS, MK_LIST_CANDIDATES): sketch + Bloom
 * gate + scan as mk_qset_run, then every genome above the thresholds is counted, compacted in ascending genome id and
 * ordered by filter_results' heap on the device.  Waits for the result (the list lives in host memory). */
int mk_qset_run_list(mk_ctx *ctx, mk_qset *qs, uint32_t nresults, uint32_t min_score, double min_intersection,
                     mk_hitlist **out);
/* ---- families: connected components of "one genome lists the other" (family.hip) ----
 * Genome i LISTS genome j when j passes filter_results' test (Miekki.cpp:381-384) for the scores of i's sequence, i.e. when
 * j is among mk_qset_run_list(from_index{i}, MK_LIST_CANDIDATES, min_score, min_intersection).  matches is symmetric,
 * intersection is not (it uses j's sizes), so i and j are LINKED when either lists the other; a FAMILY is a connected
 * component of the links (single linkage) and its LABEL the smallest id in it; a genome nobody links to is a family of one.
 * The families are kept as a union-find forest of n_ids 32-bit words in device memory of the context's GPU (mk_dev_alloc),
 * indexed by id: parent[i] <= i, a root is its own parent.  It depends on nothing but the links: not on chunks, schedules or
 * launch order.
 * mk_link_reset: parent[i] = i, every id a family of one.  Queued on the context's stream. */
int mk_link_reset(mk_ctx *ctx, uint32_t *d_parent, uint32_t n_ids);
/* One pass over the set exactly as mk_qset_run_list makes it (sketch, Bloom gate, one scan per chunk, any kind of set), but a
 * genome that passes the thresholds for query j is not reported: its id is joined with query_ids[j], the id query j stands
 * for (host array of the set's size; a query of a genome's own sequence stands for that genome's id).  d_parent must have been
 * reset (or hold earlier passes: links accumulate, a pass made twice changes nothing).  A query_ids[j] >= n_ids, or a context
 * that reports genome ids >= n_ids: MK_ERR_ARG, checked on the host before any launch -- the forest is untouched.  A stale set
 * made from the index: MK_ERR_STATE.  min_score 0 over an index with a genome of sketch_size 0: MK_ERR_UNSUPPORTED, as for
 * mk_qset_run.  Asynchronous on the context's stream; mk_stats.filter_ms carries the link pass. */
int mk_qset_run_link(mk_ctx *ctx, mk_qset *qs, const uint32_t *query_ids, uint32_t min_score, double min_intersection,
                     uint32_t *d_parent, uint32_t n_ids);
/* Joins i with d_other[i] for every i < n_ids: folds another forest over the same ids (a shard's, copied here with
 * mk_dev_copy) into d_parent.  Queued on the context's stream. */
int mk_link_merge(mk_ctx *ctx, uint32_t *d_parent, const uint32_t *d_other, uint32_t n_ids);
/* labels[i] (host) = the label of id i's family.  Waits for everything queued on the context's stream. */
int mk_link_labels(mk_ctx *ctx, const uint32_t *d_parent, uint32_t n_ids, uint32_t *labels);
/* The families of the index's own genomes in one call: a forest, sets from the index in runs of 64 ids (mk_qset_from_index: a
 * packed index is unpacked first), mk_qset_run_link per set, the labels.  labels[j] (host, mk_index_size of them) is the label
 * of local genome j, as a reported id.  An empty index: MK_OK, nothing written. */
int mk_index_families(mk_ctx *ctx, uint32_t min_score, double min_intersection, uint32_t *labels);
/* ---- nested families at several thresholds from one pass (family.hip: link_levels_kernel) ----
 * A LEVEL is a pair of thresholds; levels[0] is the loosest and neither min_score nor min_intersection may fall from one
 * level to the next.  The links of a stricter level are then a subset of those of a looser one, so every family of level
 * l + 1 lies inside one family of level l: the families NEST, and all levels come out of one all-vs-all pass.
 * Refused on the host before any launch, the forests untouched: a null argument, n_levels outside 1 .. MK_MAX_LEVELS, a level
 * whose min_score or min_intersection is below the level before it, a NaN min_intersection -- MK_ERR_ARG, the message names
 * the level -- and whatever mk_qset_run_link refuses, with its status: a query_ids[j] >= n_ids or a context that reports
 * genome ids >= n_ids (MK_ERR_ARG), levels[0].min_score 0 over an index with a genome of sketch_size 0
 * (MK_ERR_UNSUPPORTED), a stale set made from the index (MK_ERR_STATE). */
#define MK_MAX_LEVELS 8
typedef struct {
    uint32_t min_score;
    uint32_t reserved;
    double min_intersection;
} mk_level;   /* 16 bytes */
/* One pass over the set as mk_qset_run_link makes it, at levels[0]'s thresholds, over n_levels forests of n_ids words each,
 * one after the other in d_parents: forest l starts at d_parents + l * n_ids.  Each must have been reset (mk_link_reset on
 * d_parents + l * n_ids) or hold earlier passes.  A genome that passes for query j is joined with query_ids[j] in the forest
 * of the STRICTEST level the pair passes, and in that one only; passes accumulate.  Asynchronous on the context's stream;
 * mk_stats.filter_ms carries the pass. */
int mk_qset_run_link_levels(mk_ctx *ctx, mk_qset *qs, const uint32_t *query_ids, const mk_level *levels, uint32_t n_levels,
                            uint32_t *d_parents /* [n_levels][n_ids] */, uint32_t n_ids);
/* Folds the forests strict to loose: for l = n_levels - 2 down to 0, mk_link_merge of forest l + 1 into forest l, queued on
 * the context's stream.  Afterwards mk_link_labels of forest l gives exactly the labels that mk_qset_run_link over the same
 * sets at level l's thresholds gives.  Folding twice changes nothing; further passes followed by another fold are valid. */
int mk_link_fold_levels(mk_ctx *ctx, uint32_t *d_parents, uint32_t n_ids, uint32_t n_levels);
/* The nested families of the index's own genomes in one call, prepared as mk_index_families is (a batch in flight is
 * settled, a packed index is unpacked first, cold rows work): n_levels forests over the ids the context reports, one pass
 * over the index's own sets, the fold, the labels of each level.  labels[l * G + j] (host, G = mk_index_size) is the label
 * of local genome j at level l, as a reported id; with n_levels 1 it is mk_index_families' answer.  An empty index: MK_OK,
 * nothing written.  Waits for the result. */
int mk_index_hierarchy(mk_ctx *ctx, const mk_level *levels, uint32_t n_levels, uint32_t *labels /* [n_levels][G] */);
/* ---- representatives: greedy clustering of the indexed genomes in id order (rep.hip) ----
 * With LISTS and LINKED as above, ids taken in ascending order as the context reports them: genome i is a REPRESENTATIVE
 * (rep[i] = i) when no representative r < i is linked with i; otherwise rep[i] is the SMALLEST representative r < i linked
 * with i.  So rep[i] <= i, rep[rep[i]] = rep[i], no two representatives are linked, every member is linked with its own
 * representative (star clusters: a chain a - b - c whose ends are not linked is two clusters), and rep[i] lies in i's
 * family at the same thresholds.  The answer depends on the links and the id order only: not on sets, chunks, schedules or
 * launch order.  For another priority (best assembly first) reorder the index with mk_index_select first.
 * rep[j] (host, mk_index_size of them) = the representative of local genome j, as a reported id.  Prepared as
 * mk_index_families is (a batch in flight is settled, a packed index is unpacked first, cold rows work); an empty index:
 * MK_OK, nothing written; a null rep over a non-empty index or ids beyond 32 bits: MK_ERR_ARG; min_score 0 over an index
 * with a genome of sketch_size 0: MK_ERR_UNSUPPORTED -- all found on the host before any launch.  Waits for the result;
 * mk_stats.filter_ms carries the bitmap rows, the resolve and the propagate steps. */
int mk_index_representatives(mk_ctx *ctx, uint32_t min_score, double min_intersection, uint32_t *rep);
/* ---- tallies: the profile of a read set, four counters per genome (tally.hip) ----
 * For a query q, L(q) is the set of genomes that pass filter_results' test (Miekki.cpp:381-384) -- what MK_LIST_CANDIDATES
 * lists -- and, when L(q) is not empty, best(q) is the single hit of filter_results(row, 1, min_score, min_intersection)
 * (Miekki.cpp:376-397): the largest intersection and, among equal intersections, the LARGEST genome id (a heap of one is
 * replaced unless front.intersection > intersection, 387: ties replace).  The choice is by intersection, not by matches.
 * Over a set of queries genome g counts
 *   listed        the queries with g in L(q),
 *   unique        the queries with L(q) = {g},
 *   best          the queries with best(q) = g,
 *   best_matches  the sum of matches(q, g) over the queries with best(q) = g.
 * Integer sums only: the result depends on the set of queries and on nothing else -- not on chunks, schedules, how the
 * queries are split into sets, or launch order.  (A floating-point sum over reads would depend on the order; the
 * intersection serves the pass test and the choice of best(q) only, in the reference's two double operations, 382-383.)
 * The counters are an array of n_ids mk_tally in device memory of the context's GPU (mk_dev_alloc), indexed by the id the
 * context reports, as the forest of mk_link_* is; entries below genome_id_base are never touched. */
typedef struct { uint64_t listed, unique, best, best_matches; } mk_tally;   /* 32 bytes */
/* mk_tally_reset: every counter zero.  Queued on the context's stream. */
int mk_tally_reset(mk_ctx *ctx, mk_tally *d_tally, uint32_t n_ids);
/* One pass over the set exactly as mk_qset_run_list makes it (sketch, Bloom gate, one scan per chunk, any kind of set: uploaded,
 * synthetic, from the index or from columns; a mixed set part by part), but nothing per query is written or copied: the walk
 * over a chunk adds its queries to the counters.  d_tally must have been reset, or hold earlier passes: passes ACCUMULATE, a
 * pass made twice doubles its share.  Checked on the host before any launch, the counters untouched: a null argument or a
 * context that reports genome ids >= n_ids: MK_ERR_ARG; min_score 0 over an index with a genome of sketch_size 0:
 * MK_ERR_UNSUPPORTED, as for mk_qset_run_link; a stale set made from the index: MK_ERR_STATE.  An empty set or an empty
 * index: MK_OK, nothing changes.  Asynchronous on the context's stream; mk_stats.filter_ms carries the tally launches. */
int mk_qset_run_tally(mk_ctx *ctx, mk_qset *qs, uint32_t min_score, double min_intersection, mk_tally *d_tally, uint32_t n_ids);
/* out[i] (host, n_ids of them) = the counters of id i.  Waits for everything queued on the context's stream. */
int mk_tally_read(mk_ctx *ctx, const mk_tally *d_tally, uint32_t n_ids, mk_tally *out);
/* The tally of uploaded sequences in one call: counters of its own, the sequences in sets of 2^18 as mk_query_list takes
 * them, mk_qset_run_tally per set, the counters.  tally[j] (host, mk_index_size of them) is WRITTEN, not accumulated: the
 * counters of local genome j.  An empty index: MK_OK, nothing written. */
int mk_query_tally(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t min_score,
                   double min_intersection, mk_tally *tally);
/* ---- clade tallies: the profile of a read set per GROUP of genomes, five counters per clade (clade.hip) ----
 * In a collection of strain families the tallies above lose their meaning per genome: `unique` is near zero for every strain
 * (its relatives list the same reads), `best` is split among the strains by tie-break, `listed` counts a read once per
 * strain.  What a profile wants is the level above -- reads per species, family, or any grouping the caller brings.
 * A CLADE MAP gives every local genome j < G a clade number clade[j], or MK_NO_CLADE: the genome is LEFT OUT.  With L(q),
 * the intersection and the replacement rule as in the tally section above (Miekki.cpp:381-387):
 *   L'(q)     L(q) without the left-out genomes,
 *   best'(q)  the member of L'(q) with the largest intersection, among equals the largest id: filter_results(row, 1, ...)
 *             over the row with the left-out genomes removed; with nothing left out it is best(q).
 * Over a multiset of queries clade c counts
 *   listed        the queries with at least one genome of c in L'(q) -- ONCE per query, however many it lists,
 *   unique        the queries whose L'(q) is not empty and lies in c entirely,
 *   best          the queries with best'(q) in c,
 *   best_matches  the sum of matches(q, best'(q)) over those queries,
 *   hits          the pairs (q, g) with g in c and g in L'(q): the sum of the plain tally's `listed` over c's members.
 * Integer sums only: the result depends on the multiset of queries, the index, the thresholds and the map -- not on chunks,
 * schedules, how the queries are cut into sets, or launch order.  Passes ACCUMULATE, as tally passes do.
 * THE ONE RESTRICTION: among the genomes that have a clade the numbers are NON-DECREASING in j -- clades are runs of ids,
 * possibly interrupted by left-out genomes; numbers may have gaps.  It makes the per-query deduplication of `listed` and
 * `unique` free: the walk meets ids in ascending order, so a listed genome is the first of its clade for a query exactly when
 * the nearest listed genome to its left carries another number -- no memory per query, no capacity, a read that lists every
 * genome is a read like any other.  It is the layout `miekki -K <families file>` produces; a caller whose groups are
 * scattered reorders with mk_index_select first.
 * IDENTITIES.  clade[j] = j: every counter is the plain tally's and hits = listed.  One clade of all genomes: listed =
 * unique = best = the assigned reads.  Any map without left-out genomes: the sum of best is the tally's sum of best, the sum
 * of hits its sum of listed.
 * WITH A GATHER'S PICKS (mk_cover_gather): a map that numbers the picked genomes and leaves every other out re-profiles the
 * reads against the picks only -- best and unique are judged among them.
 * The counters are an array of n_clades mk_clade_tally in device memory of the context's GPU (mk_dev_alloc), indexed by clade
 * number: clade numbers are the caller's, genome_id_base plays no part in them. */
#define MK_NO_CLADE 0xffffffffu
typedef struct { uint64_t listed, unique, best, best_matches, hits; } mk_clade_tally;   /* 40 bytes */
typedef struct mk_clade_map mk_clade_map;
/* clade[j] (host, n_genomes of them) = the clade of local genome j.  Checked on the host before anything is allocated on the
 * device: a null argument, n_genomes other than mk_index_size, or a number that decreases (the message names the first genome
 * at which it does): MK_ERR_ARG.  The map owns a device copy and remembers what the ids meant, as a set from
 * mk_qset_from_index does: after mk_index_select or mk_index_import_begin a run with it is MK_ERR_STATE; genomes appended or
 * joined after the map was made are left out.  An empty index with n_genomes = 0 gives a valid map of size 0. */
int      mk_clade_map_create(mk_ctx *ctx, const uint32_t *clade, uint32_t n_genomes, mk_clade_map **out);
uint32_t mk_clade_map_size(const mk_clade_map *map);     /* 1 + the largest clade number; 0: null, or every genome left out */
void     mk_clade_map_free(mk_ctx *ctx, mk_clade_map *map);
/* mk_clade_tally_reset: every counter zero.  Queued on the context's stream. */
int mk_clade_tally_reset(mk_ctx *ctx, mk_clade_tally *d_ct, uint32_t n_clades);
/* One walk pass over the set exactly as mk_qset_run_tally makes it (any kind of set, a mixed set part by part): every chunk's
 * queries are added to the clade counters.  d_tally may be NULL; when it is given, the plain per-genome tally of the same
 * pass is added to it from the same scan, exactly as mk_qset_run_tally would add it (n_ids is checked as there; without
 * d_tally it is not looked at).  Checked on the host before any launch, the counters untouched: a null ctx, qs, map or d_ct,
 * n_clades < mk_clade_map_size(map): MK_ERR_ARG; min_score 0 over an index with a genome of sketch_size 0:
 * MK_ERR_UNSUPPORTED; a stale map or a stale set made from the index: MK_ERR_STATE.  An empty set, an empty index or a map of
 * size 0: MK_OK, the clade counters do not change (d_tally still gets its share).  Asynchronous on the context's stream;
 * mk_stats.filter_ms carries the launches. */
int mk_qset_run_clade_tally(mk_ctx *ctx, mk_qset *qs, uint32_t min_score, double min_intersection, const mk_clade_map *map,
                            mk_clade_tally *d_ct, uint32_t n_clades, mk_tally *d_tally, uint32_t n_ids);
/* out[c] (host, n_clades of them) = the counters of clade c.  Waits for everything queued on the context's stream. */
int mk_clade_tally_read(mk_ctx *ctx, const mk_clade_tally *d_ct, uint32_t n_clades, mk_clade_tally *out);
/* The clade tally of uploaded sequences in one call: a map (clade[j], host, mk_index_size of them) and counters of its own,
 * the sequences in sets of 2^18 as mk_query_tally takes them.  out[n_clades] (host) is WRITTEN, not accumulated; n_clades
 * below 1 + the largest number of the map: MK_ERR_ARG.  An empty index: MK_OK, nothing written. */
int mk_query_clade_tally(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t min_score,
                         double min_intersection, const uint32_t *clade, uint32_t n_clades, mk_clade_tally *out);
/* ---- lca: every read placed in a taxonomy by lowest common ancestor, three counters per node (lca.hip) ----
 * The tallies above say which genomes and which flat groups are in a sample; neither places a single read in a hierarchy.  A
 * read that lists three strains of one species and nothing else belongs to the species, one that lists two genera to the
 * family above them: the placement Kraken and MEGAN made standard, and the report of reads per taxon is its summary.
 * A TAXONOMY is n_nodes intervals [lo[v], hi[v]) of local genome ids, lo < hi <= n_genomes.  Any two are disjoint or one
 * contains the other; no two are equal.  They are given in PREORDER: lo non-decreasing, and among equal lo the hi strictly
 * decreasing.  A node's number is its position.  parent[v] is the smallest enclosing interval or none (MK_NO_NODE: several
 * roots are allowed); leaf[g] is the deepest node that contains genome g; a genome inside no node is LEFT OUT, exactly as
 * MK_NO_CLADE leaves a genome out.  n_nodes = 0 is a valid taxonomy that leaves every genome out.
 * With L(q), the intersection and the replacement rule as in the tally section above (Miekki.cpp:381-387):
 *   L'(q)     L(q) without the left-out genomes,
 *   best'(q)  as in the clade section: the member of L'(q) with the largest intersection, among equals the largest id; x* is
 *             its intersection,
 *   L''(q)    for a MARGIN m in 0 .. 100: { g in L'(q) : inter(g) * 100.0 >= x* * (double)(100 - m) }, in IEEE doubles with
 *             exactly these two products (no sum: nothing to contract).  m = 100 keeps all of L'(q), m = 0 the hits that tie
 *             with the best; in between it is MEGAN's top-percent rule, without which one chance hit drags a read to the root,
 *   a, b      the smallest and the largest id of L''(q),
 *   lca(q)    the deepest node that contains both: climb parent from leaf[a] until hi > b.  A climb that leaves the forest:
 *             the read is ABOVE EVERY NODE, slot n_nodes.  L'(q) empty: the read is UNASSIGNED and counts nowhere.
 * The nodes being nested intervals, the deepest node that holds a and b holds everything between them: no tree search, no
 * memory per read, no capacity.
 * Over a multiset of queries node v counts
 *   reads         the queries with lca(q) = v,
 *   best_matches  the sum of matches(q, best'(q)) over those queries,
 *   hits          the sum of |L''(q)| over those queries.
 * Integer sums only: the result depends on the multiset of queries, the index, the thresholds, the margin and the taxonomy --
 * not on chunks, schedules, how the queries are cut into sets, or launch order.  Passes ACCUMULATE.  The sums over a node's
 * subtree (a report's clade_reads) are the host's to make, from parent.
 * IDENTITIES.  A forest of disjoint roots that are a clade map's runs, m = 100: reads[v] is the clade tally's `unique`, and
 * slot n_nodes holds sum(best) - sum(unique).  One root over all genomes and a singleton leaf per genome, m = 100:
 * reads[leaf g] is the plain tally's unique[g].  Any taxonomy and margin: the sum of reads over all slots is the clade
 * tally's sum of best for the map "has a leaf / left out".  lca(q) at a smaller margin is the node at a larger margin or a
 * descendant of it.
 * The counters are an array of n_nodes + 1 mk_lca_tally in device memory of the context's GPU (mk_dev_alloc), indexed by node,
 * the last slot "above every node". */
#define MK_NO_NODE   0xffffffffu   /* no node: a root's parent, a genome that is left out, an unassigned read */
#define MK_LCA_ABOVE 0xfffffffeu   /* a read's node: above every node */
typedef struct { uint64_t reads, best_matches, hits; } mk_lca_tally;   /* 24 bytes */
typedef struct mk_taxonomy mk_taxonomy;
/* lo[v], hi[v] (host, n_nodes of each).  The host derives parent, leaf and the depths with one stack pass and checks
 * everything before anything is allocated on the device: a null argument, n_genomes other than mk_index_size, an empty or
 * out-of-range interval, a pair that overlaps without nesting, a duplicate, an order other than preorder: MK_ERR_ARG, the
 * message naming the first offending node.  The taxonomy owns device copies of leaf, parent and hi and remembers what the ids
 * meant, as a clade map does: after mk_index_select or mk_index_import_begin a run with it is MK_ERR_STATE; genomes appended
 * or joined after it was made are left out. */
int      mk_taxonomy_create(mk_ctx *ctx, const uint32_t *lo, const uint32_t *hi, uint32_t n_nodes, uint32_t n_genomes,
                            mk_taxonomy **out);
uint32_t mk_taxonomy_nodes(const mk_taxonomy *tax);      /* n_nodes; 0 for null */
/* parent_out[v] (host, n_nodes of them) = the parent of node v, MK_NO_NODE for a root.  No device work. */
int      mk_taxonomy_parents(const mk_taxonomy *tax, uint32_t *parent_out);
void     mk_taxonomy_free(mk_ctx *ctx, mk_taxonomy *tax);
/* mk_lca_tally_reset: every counter of the n_slots slots zero.  Queued on the context's stream. */
int mk_lca_tally_reset(mk_ctx *ctx, mk_lca_tally *d_lt, uint32_t n_slots);
/* One walk pass over the set exactly as mk_qset_run_tally makes it (any kind of set, a mixed set part by part): every chunk's
 * queries are added to the counters of their nodes; with a margin below 100 a query that lists more than one genome is walked
 * twice.  d_node may be NULL; when it is given (device memory, one uint32_t per query of the set) every query's node is
 * written at the query's place in the set: a node number, MK_LCA_ABOVE, or MK_NO_NODE for an unassigned read.  Checked on the
 * host before any launch, the counters untouched: a null ctx, qs, tax or d_lt, n_slots < mk_taxonomy_nodes(tax) + 1, margin
 * above 100: MK_ERR_ARG; min_score 0 over an index with a genome of sketch_size 0: MK_ERR_UNSUPPORTED; a stale taxonomy or
 * a stale set made from the index: MK_ERR_STATE.  An empty set, an empty index or a taxonomy without nodes: MK_OK, the
 * counters do not change and d_node, where given, is all MK_NO_NODE.  Asynchronous on the context's stream; mk_stats.filter_ms
 * carries the launches. */
int mk_qset_run_lca(mk_ctx *ctx, mk_qset *qs, uint32_t min_score, double min_intersection, uint32_t margin,
                    const mk_taxonomy *tax, mk_lca_tally *d_lt, uint32_t n_slots, uint32_t *d_node);
/* out[s] (host, n_slots of them) = the counters of slot s.  Waits for everything queued on the context's stream. */
int mk_lca_tally_read(mk_ctx *ctx, const mk_lca_tally *d_lt, uint32_t n_slots, mk_lca_tally *out);
/* The lca pass of uploaded sequences in one call: a taxonomy (lo, hi, host, n_nodes of each, over mk_index_size genomes) and
 * counters of its own, the sequences in sets of 2^18 as mk_query_tally takes them.  out_tally[n_nodes + 1] and, unless it is
 * NULL, out_node[nq] (both host) are WRITTEN, not accumulated.  An empty index: MK_OK, nothing written. */
int mk_query_lca(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t min_score,
                 double min_intersection, uint32_t margin, const uint32_t *lo, const uint32_t *hi, uint32_t n_nodes,
                 mk_lca_tally *out_tally, uint32_t *out_node);
/* ---- share: abundance by expectation-maximisation over the reads that several genomes share (share.hip) ----
 * The tally credits a read that lists several genomes to one of them, by filter_results' heap rule; in a family of strains
 * that is close to a coin toss, biased to the larger id.  The lca pass avoids the choice by moving such a read up a tree.
 * Neither says how many reads each genome gets.  Every read-level profiler settles that the same way (Kallisto, Salmon,
 * Centrifuge, Bracken in its own way): a read shared by several genomes is split among them in proportion to what the other
 * reads say about them, and again until the split stops moving.
 * With L(q), the intersection, best(q) and its intersection x* as in the tally section above (Miekki.cpp:381-387), for a
 * MARGIN m in 0 .. 100:
 *   K(q)   { g in L(q) : inter(g) * 100.0 >= x* * (double)(100 - m) }, in IEEE doubles with exactly these two products:
 *          mk_qset_run_lca's rule with no genome left out.  m = 100 keeps L(q), m = 0 the ties with the best.
 * A query is UNASSIGNED when K is empty (it counts in `queries` only), SETTLED when |K| = 1 (it adds 1 to unique[g]) and
 * SHARED when |K| >= 2: its ids are stored in the pool, ascending, and it adds 1 to shared[g] of every member.  N is the
 * number of assigned queries, settled plus shared; N >= 2^32 is MK_ERR_UNSUPPORTED.  The SHIFT s is bit_length(N) or any
 * larger value up to 32 (coarser weights).  Weights are 32-bit, abundances 64-bit, counted in reads with 32 fractional bits:
 *   p_0[g] = 1 for every genome; for round t = 1 .. R, R >= 1:
 *   A_t[g] = (unique[g] << 32) + the sum over the shared reads r that contain g of share_t(r, g),
 *   share_t(r, g) = floor((p_{t-1}[g] << 32) / D) with D = the sum over g' in r of p_{t-1}[g'] when D > 0; when D = 0 the
 *                   read is STARVED and every member gets floor(2^32 / |r|),
 *   p_t[g] = (uint32_t)(A_t[g] >> s).
 * Everything fits: N < 2^s, so A_t[g] <= N * 2^32 < 2^(32 + s) and p_t fits 32 bits; p << 32 and D <= |r| * 2^32 fit 64 bits;
 * one 64-by-64-bit unsigned division per entry and round.  The result is A_R[g], delta = the sum over g of
 * |A_R[g] - A_{R-1}[g]| with A_0 = 0, and the number of starved reads of round R.
 * CONSEQUENCES.  R = 1 is the equal split.  N * 2^32 - entries <= the sum over g of A_t[g] <= N * 2^32: a floor loses less
 * than one unit per stored id per round, and the loss does not build up over rounds.  Integer sums only: the result depends
 * on the multiset of lists, R and s -- not on chunks, schedules, how the queries are cut into sets, the order of the lists in
 * the pool, or launch order.  At m = 100 `unique` is the tally's unique, unique + shared its listed, N its sum of best.
 * Genome length plays no part in the split: the weights are fractions of READS, not coverage.
 * Ids are local genome numbers, as in mk_query_tally. */
typedef struct mk_sharepool mk_sharepool;
typedef struct { uint64_t queries, assigned, shared_reads, entries; } mk_share_info;   /* 32 bytes */
typedef struct { uint64_t delta, starved; uint32_t rounds, shift; } mk_share_result;   /* 24 bytes */
#define MK_SHARE_AUTO_SHIFT 0xffffffffu
/* An empty pool over the context's mk_index_size genomes, in device memory of the context's GPU.  The pool remembers what the
 * ids meant, as a clade map does: after mk_index_select or mk_index_import_begin, or with another number of genomes, a run
 * with it is MK_ERR_STATE. */
int  mk_share_create(mk_ctx *ctx, mk_sharepool **out);
void mk_share_free(mk_ctx *ctx, mk_sharepool *pool);
/* The pool empty again, a pool that failed to grow usable again.  Queued on the context's stream. */
int  mk_share_reset(mk_ctx *ctx, mk_sharepool *pool);
/* One walk pass over the set exactly as mk_qset_run_tally makes it (any kind of set, a mixed set part by part): every
 * chunk's queries are sorted into unassigned, settled and shared, a shared query walked once more to store its ids.  Passes
 * ACCUMULATE.  Checked on the host before any launch, the pool untouched: a null argument, margin above 100: MK_ERR_ARG;
 * min_score 0 over an index with a genome of sketch_size 0: MK_ERR_UNSUPPORTED; a stale pool or a stale set made from the
 * index: MK_ERR_STATE.  The pool grows as it fills: the pass reads one pair of totals per chunk back, which waits.  When it
 * cannot grow: MK_ERR_NOMEM, and the pool answers MK_ERR_STATE until mk_share_reset.  mk_stats.filter_ms carries the
 * launches. */
int  mk_qset_run_share(mk_ctx *ctx, mk_qset *qs, uint32_t min_score, double min_intersection, uint32_t margin, mk_sharepool *pool);
/* The host's own lists (from several shards, from another tool): list i is ids[offsets[i] .. offsets[i + 1]), offsets (host)
 * has n_lists + 1 entries.  A list's ids are strictly ascending and below mk_index_size; an empty list is an unassigned
 * query, a list of one id a settled one.  Anything else: MK_ERR_ARG, the list named, the pool untouched. */
int  mk_share_add_lists(mk_ctx *ctx, mk_sharepool *pool, const uint64_t *offsets, const uint32_t *ids, uint32_t n_lists);
/* What the pool holds.  No device work. */
int  mk_share_info_read(mk_ctx *ctx, const mk_sharepool *pool, mk_share_info *out);
/* The pool on the host: unique[G], shared[G], offsets[shared_reads + 1], ids[entries]; any of them may be NULL.  The order
 * of the lists is not part of the contract; the ids within a list ascend.  Waits. */
int  mk_share_export(mk_ctx *ctx, const mk_sharepool *pool, uint64_t *unique, uint64_t *shared, uint64_t *offsets, uint32_t *ids);
/* `rounds` rounds over the pool, all queued, and ONE wait at the end: abundance[G] (host) = A_R, *res = delta, starved,
 * rounds and the shift used.  rounds = 0: MK_ERR_ARG; a shift other than MK_SHARE_AUTO_SHIFT must satisfy
 * bit_length(N) <= shift <= 32, else MK_ERR_ARG.  The pool stays as it was: more reads may be added and the rounds run
 * again.  An empty pool or index: MK_OK and zeros. */
int  mk_share_rounds(mk_ctx *ctx, mk_sharepool *pool, uint32_t rounds, uint32_t shift, uint64_t *abundance, mk_share_result *res);
/* Collect and rounds of uploaded sequences in one call, with a pool of its own and the automatic shift, the sequences in
 * sets of 2^18 as mk_query_tally takes them.  abundance[G], and unless NULL unique[G], shared[G] and *info (all host), are
 * WRITTEN. */
int  mk_query_abundance(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t min_score,
                        double min_intersection, uint32_t margin, uint32_t rounds, uint64_t *abundance, uint64_t *unique,
                        uint64_t *shared, mk_share_info *info, mk_share_result *res);
/* ---- cover: breadth of coverage of the indexed genomes by a set of queries (cover.hip) ----
 * The tallies count reads per genome: depth.  A genome that shares one conserved region with a sample collects as many
 * listed reads as one that is present end to end; how much of its sketch the sample touches tells the two apart.  For a set
 * of queries Q:
 *   seen(p, v)   some q in Q has the GATED sketch value v != empty at partition p (minhash_sketch_partition_solid_kmers,
 *                Miekki.cpp:214-224 -- the sketch query_sequence scores with),
 *   covered(g)   #{ p : column_g[p] != empty and seen(p, column_g[p]) },
 *   cells        #{ (p, v) : seen(p, v) }.
 * For a set of one query, covered is that query's score row; for any set, max_q scores[q][g] <= covered(g) <=
 * min(sum_q scores[q][g], sketch_size[g]).  Integers only and no thresholds; the result depends on the set of queries and
 * on nothing else -- not on how they are split into sets, on order, or on a pass made twice.
 * NOISE FLOOR: with 8-bit fingerprints an unrelated genome is covered at about cells / (P * 256) of its sketch by chance
 * alone, so read covered(g) / sketch_size(g) against that ratio -- which is why cells is reported next to the counts.
 * The table: one bit per (partition, fingerprint value) -- bit ((p << fp_bits) + v) & 31 of 32-bit word
 * ((p << fp_bits) + v) >> 5 -- mk_cover_bytes bytes of device memory of the context's GPU (mk_dev_alloc), owned by the
 * caller as the forest of mk_link_* and the tallies are; a caller may download or upload one (32 MiB at -h 20 -f 3, 8 GiB
 * at -h 20 -f 11: a table that cannot be allocated is MK_ERR_NOMEM from mk_dev_alloc, or from mk_query_cover). */
uint64_t mk_cover_bytes(const mk_ctx *ctx);                       /* P << fp_bits >> 3; 0 for a null context */
/* mk_cover_reset: every bit zero.  Queued on the context's stream. */
int mk_cover_reset(mk_ctx *ctx, uint32_t *d_seen);
/* The set's sketch and Bloom gate as any pass makes them (any kind of set: uploaded, synthetic, from the index or from
 * columns; a mixed set part by part), and its values OR-ed into the table: passes ACCUMULATE by OR.  No scan: the slab
 * tables are not made, mk_stats.scan_launches does not move; sketch_ms carries the sketch, filter_ms the marks.  Checked on
 * the host before any launch, the table untouched: a null argument: MK_ERR_ARG; a stale set made from the index:
 * MK_ERR_STATE.  An empty set or an empty index: MK_OK, nothing changes.  Asynchronous on the context's stream. */
int mk_qset_run_cover(mk_ctx *ctx, mk_qset *qs, uint32_t *d_seen);
/* covered[j] (host, mk_index_size of them) = covered of local genome j; *cells (host, may be NULL) = the table's set bits.
 * covered may be NULL only over an empty index.  One read-only pass over the matrix whatever the number of queries; a
 * batch in flight is settled and packed cold rows are unpacked first, cold rows are read where they lie.  The marks are
 * those of the sketches as they were gated when each pass ran: an index changed between the passes and the count is the
 * caller's affair.  Waits for the result; mk_stats.filter_ms carries the pass. */
int mk_cover_count(mk_ctx *ctx, const uint32_t *d_seen, uint32_t *covered, uint64_t *cells);
/* The cover of uploaded sequences in one call: a table of its own, the sequences in sets of 2^18 as mk_query_tally takes
 * them, mk_qset_run_cover per set, mk_cover_count.  The outputs are WRITTEN, not accumulated.  An empty index: MK_OK,
 * *cells = 0 (cells may be NULL), covered not touched. */
int mk_query_cover(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t *covered, uint64_t *cells);
/* ---- winners: the winner-takes-all screen over a cover table (cover.hip; Mash screen's -w) ----
 * In a collection of related genomes covered(g) does not say which genomes are in the sample: a strain present end to end
 * covers its relatives almost as fully, because they hold the same cells, and with 8-bit fingerprints every seen cell is
 * credited to the index_size / 256 genomes that hold it on average.  After the plain count every seen cell is credited to
 * ONE genome, the best-contained of its holders, and each genome reports the cells it won.  With ss(g) = sketch_size[g]:
 *   order        genome a comes before genome b when the first of these that differs decides: covered(a) * ss(b) >
 *                covered(b) * ss(a) as an exact 64-bit product (the larger share of its own sketch covered; ss = 0 has
 *                covered = 0 and compares as share 0); the larger covered; the smaller id.  rank(g) = g's place, 0 = best.
 *   H(p, v)      { g < index_size : column_g[p] = v }, v != empty
 *   winner(p,v)  for seen(p, v) with H(p, v) not empty: its member of smallest rank
 *   won(g)       #{ p : column_g[p] != empty, seen(p, column_g[p]), winner(p, column_g[p]) = g }
 *   claimed      the seen cells that some genome holds = the sum of won.
 * won(g) <= covered(g), won(order[0]) = covered(order[0]), claimed <= min(cells, sum of covered).  Integers only, no
 * thresholds; the result depends on the table, the matrix and the order and on nothing else.  ONE ROUND, as in Mash screen:
 * the order comes from the plain counts and is not revised after the cells are dealt out.
 * mk_cover_assign: won[j] (host, mk_index_size of them) for a caller-given order: order[0 .. G) (host) a permutation of the
 * local genomes, best first.  *claimed (may be NULL) = sum of won.  Not a permutation, a null argument over a non-empty
 * index, MIEKKI_WIN_VALUES out of range: MK_ERR_ARG, checked on the host before any launch, won and *claimed untouched.
 * Empty index: MK_OK, *claimed = 0, won not touched.  One read-only pass over the matrix (two-byte fingerprints: one per
 * range of values, see DESIGN); a batch in flight is settled and packed cold rows are unpacked first.  Waits;
 * mk_stats.filter_ms carries the pass. */
int mk_cover_assign(mk_ctx *ctx, const uint32_t *d_seen, const uint32_t *order, uint32_t *won, uint64_t *claimed);
/* count pass, the order of the definition (sorted on the host), mk_cover_assign: covered, won (host, G each), cells, claimed
 * (may be NULL).  A null argument is refused before the count pass: nothing is written.  Empty index: *cells as
 * mk_cover_count gives it, *claimed = 0. */
int mk_cover_winners(mk_ctx *ctx, const uint32_t *d_seen, uint32_t *covered, uint32_t *won, uint64_t *cells, uint64_t *claimed);
/* uploaded sequences in one call, as mk_query_cover takes them; the outputs are WRITTEN.  Empty index: MK_OK, *cells =
 * *claimed = 0, covered and won not touched. */
int mk_query_cover_winners(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq,
                           uint32_t *covered, uint32_t *won, uint64_t *cells, uint64_t *claimed);
/* ---- taxon cover: distinct covered cells per node of a taxonomy (taxcover.hip; KrakenUniq's unique k-mer counts) ----
 * A node of a taxonomy can collect many reads from one conserved region: reads per node do not tell a present species from a
 * false positive, the number of DISTINCT cells of the taxon that the sample touches does.  Per genome that is covered against
 * sketch_size; above the leaves the per-genome numbers do not add up -- the strains of a species share most of their cells,
 * their sum counts a shared cell once per strain, their maximum ignores what the best strain lacks.  With seen, cells and
 * empty as in the cover section and a taxonomy as in the lca section, node n being the interval [lo[n], hi[n]) of local ids:
 *   H(n, p)     { column_g[p] : lo[n] <= g < hi[n], column_g[p] != empty }     the values node n holds at partition p,
 *   held(n)     sum over p of |H(n, p)|                                        the node's pan-sketch size,
 *   covered(n)  sum over p of |{ v in H(n, p) : seen(p, v) }|.
 * Both go up to P * 2^fp_bits: 64-bit counters.  Integers only and exact: the result depends on the table, the matrix and the
 * taxonomy and on nothing else -- not on row chunks, launch order or which kernel path a node takes; held depends on the index
 * and the taxonomy only.
 * IDENTITIES.  A node of one genome g: held = sketch_size[g], covered = mk_cover_count's covered[g].  A root over all genomes:
 * covered = mk_cover_winners' claimed.  Any node, for held and for covered alike: max over its children <= value(n) <= sum
 * over its children + the same count over the node's genomes that lie in no child.  covered(n) <= held(n).  An all-ones table:
 * covered = held (the bit of `empty` counts for nothing, the zero padding of the rows holds no value 0); an all-zero table:
 * covered = 0, held unchanged.
 * NOISE FLOOR: with 8-bit fingerprints an unrelated node is covered at about cells / (P * 256) of its held by chance alone --
 * the ratio of the cover section: read covered(n) / held(n) against the same number.
 * COST: the pass reads sum over the nodes of width >= 2 of width * P * W bytes, one read of the matrix per level of the
 * taxonomy; cold rows are read where they lie, once per level. */
typedef struct { uint64_t held, covered; } mk_node_cover;   /* 16 bytes */
/* out[v] (host, mk_taxonomy_nodes of them) = held and covered of node v: WRITTEN, not accumulated.  *cells (host, may be NULL) =
 * the table's set bits.  d_seen may be NULL: only held is computed, covered is written as 0 and *cells as 0.  Nodes of one
 * genome take sketch_size and one mk_cover_count pass (none when the taxonomy has no such node), every other node the node
 * pass.  A batch in flight is settled and packed cold rows are unpacked first, as for mk_cover_count.  Checked on the host
 * before any launch, the outputs untouched: a null ctx or tax, a null out over a taxonomy with nodes: MK_ERR_ARG ("null
 * argument"); a taxonomy made for another context: MK_ERR_ARG; MIEKKI_TAXCOVER_ROWS or MIEKKI_TAXCOVER_WIDE (DESIGN) with a value
 * they do not take: MK_ERR_ARG naming the switch; a stale taxonomy (after mk_index_select / mk_index_import_begin):
 * MK_ERR_STATE.  A taxonomy without nodes -- the only one an empty index has --: MK_OK, out untouched, *cells the table's.
 * Genomes appended after the taxonomy was made are left out, as for lca.  Waits for the result; mk_stats.filter_ms carries
 * the kernels. */
int mk_taxonomy_cover(mk_ctx *ctx, const mk_taxonomy *tax, const uint32_t *d_seen, mk_node_cover *out, uint64_t *cells);
/* The node cover of uploaded sequences in one call: a taxonomy (lo, hi, host, n_nodes of each, over mk_index_size genomes) and
 * a table of its own, the sequences marked in sets of 2^18 as mk_query_cover marks them, then mk_taxonomy_cover.  The outputs
 * are WRITTEN.  An empty index: MK_OK, *cells = 0 (cells may be NULL), out not touched. */
int mk_query_taxonomy_cover(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq, const uint32_t *lo,
                            const uint32_t *hi, uint32_t n_nodes, mk_node_cover *out, uint64_t *cells);
/* ---- taxon markers: the cells of a taxon and of nothing outside it (markers.hip; Kraken's k-mer LCA, MetaPhlAn's clade markers) ----
 * The taxon cover counts a cell for a node as soon as any genome of the node holds it, whoever else holds it too: with related
 * genomes, and with 8-bit fingerprints at all, most of a node's covered cells are held outside the node as well.  Here every
 * held cell belongs to ONE slot, the deepest node that contains all its holders.  With seen, cells and empty as in the cover
 * section and a taxonomy as in the lca section (leaf[g], parent, node n the interval [lo[n], hi[n]) of local ids):
 *   H'(p, v)      { g < index_size : leaf[g] != MK_NO_NODE, column_g[p] = v }, for v != empty.  A genome inside no node is left
 *                 out, as lca and the clade tally leave it out; so are genomes appended after the taxonomy was made.
 *   owner(p, v)   for a non-empty H'(p, v) with smallest id a and largest id b: the deepest node that contains both -- climb
 *                 parent from leaf[a] until hi > b.  A climb that leaves the forest gives "above every node", slot n_nodes.
 *   specific(n)   #{ (p, v) : owner(p, v) = n }
 *   covered(n)    #{ (p, v) : owner(p, v) = n, seen(p, v) }
 * Both are 64-bit, integers and exact: the result depends on the matrix, the table and the taxonomy and on nothing else -- not
 * on row chunks, value ranges, launch order or which kernel path a row takes; specific depends on the index and the taxonomy
 * only.  Subtree sums are the host's to make, from parent, as for lca's clade_reads: clade_specific(n) is the number of cells
 * all of whose holders that have a leaf lie inside n.
 * IDENTITIES.  The sum of specific over all slots is the number of distinct held cells of the genomes that have a leaf: with one
 * root over all genomes mk_taxonomy_cover's held(root), and the above slot is 0.  When every genome has a leaf, the sum of
 * covered over all slots is mk_cover_winners' claimed.  clade_specific(n) <= held(n) and clade_covered(n) <= covered(n) of
 * mk_taxonomy_cover, equalities for a root when no genome outside it has a leaf.  A leaf of one genome g: specific <=
 * sketch_size[g], with equality in an index of one genome; the cells of two identical sibling genomes belong to their parent,
 * the leaves get 0.  An all-ones table: covered = specific; an all-zero table or d_seen = NULL: covered = 0, specific
 * unchanged.  For every node clade_specific(n) is the count made without minimum and maximum: the cells held inside [lo, hi)
 * and by no genome outside it that has a leaf.
 * COST: one read of the matrix at one-byte fingerprints; at two bytes a row passes once per range of values that fits LDS. */
typedef struct { uint64_t specific, covered; } mk_node_markers;   /* 16 bytes */
/* out[v] (host, n_slots >= mk_taxonomy_nodes + 1 of them; the last one used is the slot above every node) = specific and covered
 * of node v: WRITTEN, not accumulated.  *cells (host, may be NULL) = the table's set bits, 0 with a NULL table.  d_seen may be
 * NULL: only specific is computed.  A batch in flight is settled and packed cold rows are unpacked first, as for
 * mk_cover_count; cold rows are read where they lie.  Checked on the host before any launch, the outputs untouched: a null ctx,
 * tax or out: MK_ERR_ARG ("null argument"); too few slots: MK_ERR_ARG; a taxonomy made for another context: MK_ERR_ARG;
 * MIEKKI_MARK_ROWS, MIEKKI_MARK_VALUES, MIEKKI_MARK_FILTER or MIEKKI_MARK_TOUCHED (DESIGN) with a value they do not take:
 * MK_ERR_ARG naming the switch; a stale taxonomy (after mk_index_select / mk_index_import_begin): MK_ERR_STATE.  A taxonomy
 * without nodes, or an empty index: MK_OK, out[0] (the above slot) zero.  Waits for the result; mk_stats.filter_ms carries
 * the pass. */
int mk_taxonomy_markers(mk_ctx *ctx, const mk_taxonomy *tax, const uint32_t *d_seen, mk_node_markers *out, uint32_t n_slots,
                        uint64_t *cells);
/* The markers of uploaded sequences in one call: a taxonomy (lo, hi, host, n_nodes of each, over mk_index_size genomes) and a
 * table of its own, the sequences marked in sets of 2^18 as mk_query_cover marks them, then mk_taxonomy_markers.  The outputs
 * are WRITTEN.  An empty index: MK_OK, out[0] zero, *cells = 0 (cells may be NULL). */
int mk_query_taxonomy_markers(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq, const uint32_t *lo,
                              const uint32_t *hi, uint32_t n_nodes, mk_node_markers *out, uint32_t n_slots, uint64_t *cells);
/* ---- depth: depth of coverage of the indexed genomes by a set of queries (depth.hip; Mash screen's median multiplicity) ----
 * listed / best count reads and scale with genome length; covered is an OR and forgets every repeat.  A read that contains a
 * genome's minimum k-mer of partition p has that k-mer as its own minimum of p, so the number of reads whose gated sketch
 * holds column_g[p] at p IS the depth at that k-mer.  For a set of queries Q (a multiset: a query given twice counts twice):
 *   mult(p, v)   min(255, #{ q in Q : the GATED sketch of q (minhash_sketch_partition_solid_kmers, Miekki.cpp:214-224) has
 *                value v != empty at partition p }); MK_DEPTH_MAX is 255,
 *   covered(g)   #{ p : column_g[p] != empty and mult(p, column_g[p]) > 0 } -- mk_cover_count's covered for the same queries,
 *   sum(g)       the sum of mult(p, column_g[p]) over those p, 64 bits; the mean depth is sum / covered, which the caller divides,
 *   median(g)    the LOWER median of those covered(g) values: sorted ascending, the element of index (covered - 1) / 2;
 *                equally the largest t in 1..255 with #{ p : column_g[p] != empty, mult(p, column_g[p]) >= t } >=
 *                covered(g) / 2 + 1; 0 when covered(g) = 0,
 *   cells        #{ (p, v) : mult > 0 },
 *   saturated    #{ (p, v) : mult = 255 }.
 * Passes ACCUMULATE with saturation: a pass made twice doubles the multiplicities up to the cap, as a tally pass doubles its
 * share and unlike the cover's OR.  min(255, count) does not depend on the order of the increments: the result is a function
 * of the multiset of queries and the matrix and of nothing else -- not of slices, chunks, launch order or how a caller cuts
 * its reads into sets.  Integers only, no thresholds.  THE CAP: a median of 255 means "255 or more", which is why saturated
 * is reported.  NOISE FLOOR: with 8-bit fingerprints read median only where covered(g) / sketch_size(g) stands clear of
 * cells / (P * 256), the share of its sketch an unrelated genome is covered at by chance.
 * The table: one byte per (partition, fingerprint value) at byte index (p << fp_bits) + v -- mk_depth_bytes bytes of device
 * memory of the context's GPU (mk_dev_alloc), owned by the caller as the cover table is; a caller may download or upload one
 * (128 KiB at -h 9 -f 3, 256 MiB at -h 20 -f 3, 8 GiB at -h 17 -f 11, 64 GiB at -h 20 -f 11: a table that cannot be
 * allocated is MK_ERR_NOMEM from mk_dev_alloc, or from mk_query_depth). */
#define MK_DEPTH_MAX 255u
typedef struct { uint64_t sum; uint32_t covered; uint32_t median; } mk_depth;   /* 16 bytes */
uint64_t mk_depth_bytes(const mk_ctx *ctx);                       /* P << fp_bits; 0 for a null context */
/* mk_depth_reset: every byte zero.  Queued on the context's stream. */
int mk_depth_reset(mk_ctx *ctx, uint8_t *d_mult);
/* The set's sketch and Bloom gate as any pass makes them (any kind of set: uploaded, synthetic, from the index or from
 * columns; a mixed set part by part), and one added to the byte of each of its values, up to 255.  No scan: the slab tables
 * are not made, mk_stats.scan_launches does not move; sketch_ms carries the sketch, filter_ms the marks.  Checked on the host
 * before any launch, the table untouched: a null argument: MK_ERR_ARG; a stale set made from the index: MK_ERR_STATE.  An
 * empty set or an empty index: MK_OK, nothing changes.  Asynchronous on the context's stream. */
int mk_qset_run_depth(mk_ctx *ctx, mk_qset *qs, uint8_t *d_mult);
/* depth[j] (host, mk_index_size of them) = sum, covered and median of local genome j, WRITTEN, not accumulated; *cells and
 * *saturated (host, either may be NULL) = the table's non-zero bytes and its bytes of 255.  depth may be NULL only over an
 * empty index, where *cells and *saturated are still the table's.  Nine read-only passes over the matrix whatever the number
 * of queries (pass 0: covered and sum; eight bisection steps for the median, none waited for on the host); a batch in flight
 * is settled and packed cold rows are unpacked first, cold rows are read where they lie, once per pass.  Waits for the
 * result; mk_stats.filter_ms carries the passes. */
int mk_depth_profile(mk_ctx *ctx, const uint8_t *d_mult, mk_depth *depth, uint64_t *cells, uint64_t *saturated);
/* The depth of uploaded sequences in one call: a table of its own, the sequences in sets of 2^18 as mk_query_cover takes
 * them, mk_qset_run_depth per set, mk_depth_profile.  The outputs are WRITTEN, not accumulated.  An empty index: MK_OK,
 * *cells = *saturated = 0 (either may be NULL), depth not touched. */
int mk_query_depth(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq,
                   mk_depth *depth, uint64_t *cells, uint64_t *saturated);
/* ---- gather: which few genomes, taken together, explain the sample (gather.hip; sourmash's gather: the greedy minimum set
 * cover) ----
 * covered, won and depth answer "how much of genome g does the sample touch?".  The winners' order comes from the plain
 * counts and is never revised: the second-best strain of a family that is present still ranks above every genome of a less
 * abundant family.  Here every pick is judged against what the picks before it left over.  seen, covered, cells and empty are
 * the cover section's; G = mk_index_size:
 *   live_0       = seen,
 *   rem_r(g)     #{ p : column_g[p] != empty and live_r(p, column_g[p]) }, so rem_0 = covered,
 *   round r      w_r = the genome of largest rem_r, among equals the smallest id (the 64-bit key rem << 32 | ~id, maximised).
 *                Stop if rem_r(w_r) < min_new, or if r == max_picks when max_picks != 0.  Otherwise the pick's fresh =
 *                rem_r(w_r), and live_{r+1} is live_r without the cells (p, column_w[p]) that were live.
 * Per pick: genome = the REPORTED id (local id + genome_id_base), fresh, covered = rem_0 of the pick (its overlap with the
 * whole sample), sketch_size, and depth_sum = the sum of mult(p, v) over the cells the pick struck when a depth table is
 * given (64 bits; depth_sum / fresh is the mean depth of what the genome alone explains), else 0.  explained = the sum of
 * fresh.  fresh never increases from one pick to the next; picks[0] is the arg-max of covered and its fresh equals its
 * covered; no genome is picked twice; with min_new = 1 and no cap explained equals mk_cover_winners' claimed; there are at
 * most G rounds.  Integers only: the result is a function of the table, the matrix, min_new and max_picks and of nothing
 * else -- not of chunks, launch order or the rounds queued per host wait (MIEKKI_GATHER_ROUNDS, 32 unless set;
 * MIEKKI_GATHER_RECOUNT=1 recounts rem with the count pass after every pick instead of subtracting the struck rows' matches:
 * the same picks).  NOISE FLOOR: with 8-bit fingerprints an unrelated genome's rem is about sketch_size * live cells /
 * (P * 256); min_new has to stand clear of it, or index with 16-bit fingerprints.
 * mk_cover_gather: d_seen and d_mult (may be NULL) are the caller's and are NOT modified: the call works on a copy of d_seen
 * of its own, mk_cover_bytes large; a copy that cannot be allocated is MK_ERR_NOMEM, reported before anything is written.
 * picks (host): room for max_picks, or for G when max_picks = 0; *n_picks = the picks made; *cells, *explained (either may be
 * NULL).  A null ctx, d_seen or n_picks, null picks over a non-empty index, min_new = 0 (the loop would not end): MK_ERR_ARG,
 * checked on the host before any launch, the outputs untouched.  An empty index: MK_OK, *n_picks = 0, *explained = 0, *cells
 * as mk_cover_count gives it.  A batch in flight is settled and packed cold rows are unpacked first, as for mk_cover_count;
 * cold rows are read where they lie.  The take step's count of struck cells must equal the fresh the pick step found: a
 * mismatch is the library disagreeing with itself, MK_ERR_STATE with a message and no picks returned.  Waits for the result;
 * mk_stats.filter_ms carries the kernels. */
typedef struct { uint32_t genome, fresh, covered, sketch_size; uint64_t depth_sum; } mk_pick;   /* 24 bytes */
int mk_cover_gather(mk_ctx *ctx, const uint32_t *d_seen, const uint8_t *d_mult, uint32_t min_new, uint32_t max_picks,
                    mk_pick *picks, uint32_t *n_picks, uint64_t *cells, uint64_t *explained);
/* uploaded sequences in one call, as mk_query_cover_winners takes them: a table of its own -- and, with_depth != 0, a depth
 * table of its own -- the sequences in sets of 2^18, then mk_cover_gather.  The outputs are WRITTEN.  Empty index: MK_OK,
 * *n_picks = 0, *cells = *explained = 0, picks not touched. */
int mk_query_cover_gather(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, uint32_t nq, int with_depth,
                          uint32_t min_new, uint32_t max_picks, mk_pick *picks, uint32_t *n_picks,
                          uint64_t *cells, uint64_t *explained);
/* ---- panel: the cover of up to eight samples with one pass over the matrix (panel.hip) ----
 * A cohort -- a run's barcodes, a time series, a study's samples -- is screened against one index; with the cover that is
 * one table and one pass over the matrix per sample.  A PANEL is up to MK_PANEL_SLOTS (8) samples Q_0 .. Q_7, each a set of
 * queries in the cover section's sense; with seen_s, covered_s and cells_s the cover section's seen, covered and cells for Q_s:
 *   table          one byte per (partition, fingerprint value) at byte index (p << fp_bits) + v; bit s of that byte is set
 *                  iff seen_s(p, v),
 *   covered[s][g]  covered_s(g),
 *   cells[s]       cells_s -- exactly what mk_cover_count gives for a cover table marked with Q_s alone.
 * Integers only, no thresholds.  Marks ACCUMULATE by OR: a pass made twice changes nothing, and the result depends on the
 * samples and the matrix, not on chunks, launch order or how a caller cuts a sample into sets.  NOISE FLOOR: the cover
 * section's, per slot: read covered[s][g] / sketch_size(g) against cells[s] / (P * 256) with 8-bit fingerprints.
 * The table: mk_panel_bytes bytes of device memory of the context's GPU (mk_dev_alloc), the size of a depth table, owned by
 * the caller as the cover table is; a caller may download or upload one. */
#define MK_PANEL_SLOTS 8u
uint64_t mk_panel_bytes(const mk_ctx *ctx);                      /* P << fp_bits; 0 for a null context */
/* mk_panel_reset: every byte zero.  Queued on the context's stream. */
int mk_panel_reset(mk_ctx *ctx, uint8_t *d_panel);
/* The set's sketch and Bloom gate as mk_qset_run_cover makes them (any kind of set; a mixed set part by part), and bit `slot`
 * OR-ed into the byte of each of its values.  No scan: mk_stats.scan_launches does not move; sketch_ms carries the sketch,
 * filter_ms the marks.  Checked on the host before any launch, the table untouched: a null argument or slot >=
 * MK_PANEL_SLOTS: MK_ERR_ARG; a stale set made from the index: MK_ERR_STATE.  An empty set or an empty index: MK_OK, nothing
 * changes.  Asynchronous on the context's stream. */
int mk_qset_run_panel(mk_ctx *ctx, mk_qset *qs, uint32_t slot, uint8_t *d_panel);
/* covered[s * G + j] (host, n_slots * mk_index_size words) = covered of local genome j by slot s, WRITTEN, not accumulated;
 * cells[s] (host, n_slots words, may be NULL) = the table's bytes with bit s set.  ONE read-only pass over the matrix whatever
 * n_slots is; slots >= n_slots are not reported and their bits may be anything.  n_slots = 0 or > MK_PANEL_SLOTS, a null
 * ctx or d_panel, or a null covered over a non-empty index: MK_ERR_ARG before any launch.  Over an empty index: MK_OK, cells
 * is still the table's, covered is not touched.  A batch in flight is settled and packed cold rows are unpacked first, cold
 * rows are read where they lie, as for mk_cover_count.  Waits for the result; mk_stats.filter_ms carries the pass. */
int mk_panel_count(mk_ctx *ctx, const uint8_t *d_panel, uint32_t n_slots, uint32_t *covered, uint64_t *cells);
/* d_seen (device, mk_cover_bytes bytes) is WRITTEN with slot `slot`'s plane in the cover table's layout: a panel sample goes
 * on to mk_cover_winners or mk_cover_gather without being marked again.  A null argument or slot >= MK_PANEL_SLOTS:
 * MK_ERR_ARG.  Queued on the context's stream. */
int mk_panel_slot(mk_ctx *ctx, const uint8_t *d_panel, uint32_t slot, uint32_t *d_seen);
/* Any number of samples of uploaded sequences in one call: sample s is seqs[starts[s] .. starts[s + 1]) (starts: n_samples + 1
 * entries, non-decreasing from 0).  One table of its own, the samples in groups of eight: per group a reset, the marks (in
 * sets of 2^18 as mk_query_cover takes them) and one count pass.  covered[n_samples][G] and cells[n_samples] (may be NULL) are
 * WRITTEN.  A decreasing starts or a null argument: MK_ERR_ARG.  n_samples = 0 or an empty index: MK_OK, the cells entries
 * are written as 0, covered is not touched. */
int mk_query_panel(mk_ctx *ctx, const char *const *seqs, const uint64_t *lens, const uint64_t *starts,
                   uint32_t n_samples, uint32_t *covered, uint64_t *cells);
/* A set keeps its sketch, Bloom gate result and schedule tables until the index changes
 * (genomes appended / imported, Bloom cells written); this forces the next run to redo
 * them anyway (bench.py: a timed step is a complete pass). */
int mk_qset_invalidate(mk_ctx *ctx, mk_qset *qs);
/* Raw scores of queries [q_begin, q_end) of the set into d_scores[(q_end-q_begin)][G]. */
int mk_qset_scores(mk_ctx *ctx, mk_qset *qs, uint32_t q_begin, uint32_t q_end, uint32_t *d_scores);
/* active partitions per query after the last run/scores call */
int mk_qset_active(mk_ctx *ctx, mk_qset *qs, uint32_t *active);
int mk_sync(mk_ctx *ctx);

/* ---- several GPUs in one process (the `miekki` binary; Miekki.cpp:546-581, 430-480 scale
 * inside one executable with -t).  One context per GPU, genomes sharded in list order. ---- */

int mk_device_count(void);                                  /* visible HIP devices (0 without a GPU) */
/* ids this context reports = local index + base; may be set after the build, once the
 * number of genomes the shards before it kept is known. */
int mk_set_genome_id_base(mk_ctx *ctx, uint32_t base);
/* Device memory on the context's GPU for callers without a GPU runtime of their own. */
int mk_dev_alloc(mk_ctx *ctx, uint64_t bytes, void **d_out);
void mk_dev_free(mk_ctx *ctx, void *d_ptr);
int mk_dev_upload(mk_ctx *ctx, void *d_dst, const void *src, uint64_t bytes);
int mk_dev_download(mk_ctx *ctx, void *dst, const void *d_src, uint64_t bytes);
/* d_src on src's GPU -> d_dst on dst's GPU: a peer DMA over xGMI, ordered behind src's
 * queued work; complete on return. */
int mk_dev_copy(mk_ctx *dst, void *d_dst, mk_ctx *src, const void *d_src, uint64_t bytes);
/* Bloom cells [begin, end) to / from device memory of the context's GPU. */
int mk_index_export_bloom_device(mk_ctx *ctx, uint64_t begin, uint64_t end, uint8_t *d_dst);
int mk_index_import_bloom_device(mk_ctx *ctx, uint64_t begin, uint64_t end, const uint8_t *d_src);
/* First-writer fold of a genome-sharded build (the reference's single filter keeps the byte of a
 * cell's first inserter in genome order, Miekki.cpp:125-129): cells [begin, end) of this context
 * keep their byte where it is non-zero and take d_later's otherwise.  Called on the first shard
 * with the filters of the later shards in shard order; begin must be a multiple of 16. */
int mk_index_merge_bloom_device(mk_ctx *ctx, uint64_t begin, uint64_t end, const uint8_t *d_later);
/* bytes of the Bloom table a 2k-bit k-mer can reach (everything above stays zero) */
uint64_t mk_bloom_reachable_bytes(const mk_ctx *ctx);

/* ---- one process per GPU: the collectives of the genome-sharded index, on RCCL over xGMI --------------
 * The reference scales inside one executable (-t threads, main.cpp:190-196; Miekki.cpp:546-581, 430-480) and has
 * no distributed backend; SURVEY.md 8e defines the multi-GPU form: rank r owns a contiguous genome range, the
 * Bloom filter is made global once after the build, and a query batch needs ONE exchange step -- ncclGather
 * (rccl.h:745) of the per-query heap-entrant rows (mk_qset_run_compact) to the merging rank.  librccl is bound at
 * run time (a process that already holds a copy, e.g. PyTorch's, keeps using it; MIEKKI_RCCL_LIB names one);
 * single-GPU users never load it.  One communicator per context; every call below is COLLECTIVE: all ranks make
 * it, in the same order.  Device pointers (d_*) are memory of the context's GPU; the collectives are queued on
 * the context's stream like its kernels (mk_sync waits), so a gather needs no host wait after the scan. */
typedef struct mk_comm mk_comm;
#define MK_COMM_ID_BYTES 128
/* rank 0 draws the id (ncclGetUniqueId) and hands it to the other ranks by any means (a file, the launcher's
 * store, an environment variable); then every rank creates its communicator (ncclCommInitRank). */
int mk_comm_unique_id(uint8_t *id /* MK_COMM_ID_BYTES */);
/* (This RCCL build prints a version banner on stdout from rank 0's first communicator.  With MIEKKI_COMM_BANNER_TO_STDERR=1
 * in the environment mk_comm_create points descriptor 1 at descriptor 2 while the communicator initialises -- process-wide,
 * for as long as the slowest rank takes to arrive: only for programs that own their stdout, like the `miekki` binary and
 * bench.py, which set it themselves.  Without it nothing is redirected.) */
int mk_comm_create(mk_ctx *ctx, int rank, int world, const uint8_t *id, mk_comm **out);
void mk_comm_destroy(mk_comm *comm);
int mk_comm_rank(const mk_comm *comm);
int mk_comm_world(const mk_comm *comm);
/* ncclGather / ncclAllGather / ncclBroadcast of plain bytes; d_recv holds world * bytes (gather: on root only). */
int mk_comm_gather(mk_comm *comm, const void *d_send, uint64_t bytes, void *d_recv, int root);
int mk_comm_allgather(mk_comm *comm, const void *d_send, uint64_t bytes, void *d_recv);
int mk_comm_broadcast(mk_comm *comm, void *d_buf, uint64_t bytes, int root);
int mk_comm_allreduce_max_f64(mk_comm *comm, double *d_values, uint32_t n);
int mk_comm_barrier(mk_comm *comm);                                /* waits on the host, too */
/* The single exchange step: every rank's exchange rows (`words` 64-bit words, what mk_qset_run_compact wrote) ->
 * d_recv[world][words] on root, rank-major = shard order = genome order: the layout mk_merge_compact takes. */
int mk_comm_gather_rows(mk_comm *comm, const uint64_t *d_rows, uint64_t words, uint64_t *d_recv, int root);
/* Once after the build.  The reference has ONE Bloom filter and a cell keeps the byte of its first inserter in
 * genome order (Miekki.cpp:125-129); with contiguous shards in rank order that is the lowest rank whose cell is
 * non-zero: a MIN all-reduce over (rank << 8 | byte), in place on the context's filter, byte-exact. */
int mk_comm_sync_bloom(mk_comm *comm);
/* Once after the build: all-gathers how many genomes every rank holds and their sketch_size / genome_size, sets
 * this context's genome id base to the genomes of the ranks before it (ids = those of a single-process run) and
 * hands all sizes to the merge (mk_merge_set_sizes).  id_base / total may be NULL. */
int mk_comm_share_sizes(mk_comm *comm, uint32_t *id_base, uint32_t *total);
/* mk_qset_run_compact with its exchange step folded in: the rows of queries that are finished leave for `root` on
 * the communicator's own stream WHILE the next chunk of queries is scanned (sets of >= 4096 queries go in four
 * blocks, MIEKKI_EXCHANGE_BLOCKS; a smaller set is one ncclGather).  d_rows[nq][1 + cap] on every rank,
 * d_recv[world][nq][1 + cap] on root (NULL elsewhere).  On return everything is queued and the context's stream
 * waits for the exchange: mk_merge_compact(ctx, d_recv, world, ...) may follow at once. */
int mk_qset_run_compact_gather(mk_ctx *ctx, mk_comm *comm, mk_qset *qs, uint32_t nresults, uint32_t min_score,
                               double min_intersection, uint32_t cap, uint64_t *d_rows, uint64_t *d_recv, int root);

/* ---- exact mode (ground_truth_batch, Miekki.cpp:792-859) ------------------- */

/* genome: contig sequences as ground_truth_batch delimits them (Miekki.cpp:803-822);
 * for each query: |A n B| and |B| + |A \ B| over distinct canonical k-mers. */
int mk_exact(mk_ctx *ctx, const char *const *contigs, const uint64_t *contig_lens,
             uint32_t n_contigs, const char *const *queries, const uint64_t *query_lens,
             uint32_t nq, uint64_t *inter, uint64_t *uni);
/* The same in two steps, for callers that verify several batches of queries against one
 * genome file (the reference rebuilds its unordered_set at every flush of 100 pending
 * queries, Miekki.cpp:745-748, ~7 s each): the genome's k-mer set stays resident on the
 * context until the next load.  Any number of contigs and queries per call. */
int mk_exact_load_genome(mk_ctx *ctx, const char *const *contigs, const uint64_t *contig_lens,
                         uint32_t n_contigs);
int mk_exact_query(mk_ctx *ctx, const char *const *queries, const uint64_t *query_lens, uint32_t nq,
                   uint64_t *inter, uint64_t *uni);

#ifdef __cplusplus
}
#endif
#endif
