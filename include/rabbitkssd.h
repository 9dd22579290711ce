/*
 * rabbitkssd.h -- C ABI of the MI355X-native sketch + distance engine (librabbitkssd.so).
 *
 * Drop-in boundary for RabbitKSSD's hot path.  The reference has no FFI of its own; the
 * seams this ABI replaces are four C++ free functions and the arithmetic inside them
 * (citations are file:line into the reference tree):
 *
 *   rk_params_init         <- initParameter             src/common.cpp:35-78
 *   rk_filter_create       <- shuffled_map construction  src/sketch.cpp:336-345
 *   rk_sketch_batch        <- per-genome loop of sketchFastaFile
 *                                                        src/sketch.cpp:455-566 (and :173-238)
 *   rk_sketch_batch_ex     <- per-file loop of sketchFastqFile   src/sketch.cpp:741-866
 *   rk_index_build         <- transSketches              src/sketch.cpp:970-1017 (32-bit), :904-969 (64-bit)
 *   rk_index_import/export <- .dict/.index load/store    src/dist.cpp:86-129, src/sketch.cpp:991-1011
 *   rk_dist_rows           <- row loop of index_tridist  src/dist.cpp:174-258
 *                             row loop of index_dist     src/dist.cpp:560-692 (without -N)
 *   rk_topn_rows           <- -N max-heap of index_dist  src/dist.cpp:599,625-640,683-689
 *   rk_dist_topn           <- row loop of index_dist with -N (counting, epilogue and heap per
 *                             query row)             src/dist.cpp:560-692
 *   rk_cluster_rows        <- row loop of index_tridist  src/dist.cpp:174-258, followed by the union-find its
 *                             users run over the printed pairs (the reference has no clustering of its own)
 *   rk_forest_rows         <- the same row loop, followed by the Kruskal its users run over the printed pairs
 *   rk_greedy_rows         <- the same row loop, followed by the greedy incremental clustering its users run over the
 *                             printed pairs (the rule of CD-HIT, Li & Godzik 2006, and of clust-greedy in RabbitTClust, the
 *                             reference's sibling tool; the reference itself has no clustering)
 *   rk_dbscan_rows         <- the same row loop, followed by the DBSCAN its users run over the printed pairs (Ester et al.
 *                             1996; min_pts as scikit-learn's min_samples; the reference itself has no clustering)
 *   rk_mreach_rows         <- the same row loop, followed by the mutual-reachability spanning forest of HDBSCAN* its users
 *                             build over the printed pairs (Campello, Moulavi & Sander 2013)
 *   rk_medoid_rows         <- the same row loop, followed by what its users compute per cluster of any of the above from the
 *                             printed pairs: the most central member (the representative dRep, GTDB and galah print), the
 *                             cluster's density and weakest pair, every genome's nearest genome outside its cluster
 *   rk_assign_rows         <- row loop of index_dist     src/dist.cpp:560-692 (without -N), followed by what its users do
 *                             with the printed pairs of new genomes against a clustered collection: the cluster of the
 *                             nearest labelled reference, its support, the runner-up cluster, novelty
 *
 * Conventions
 *   - plain C types only; every call returns 0 on success or a negative rk_status and
 *     never calls exit(); rk_last_error(ctx) returns a message for the last failure on
 *     that context.
 *   - pointers are HOST pointers unless the parameter name ends in _dev.
 *   - objects (rk_filter, rk_sketches, rk_index) are library-owned, device-resident and
 *     freed with their *_free function; buffers the caller receives from the library are
 *     released with rk_free_host.  Nothing crosses allocators.
 *   - calls without a `stream` argument are synchronous at return.  *_dev calls are
 *     asynchronous on the given HIP stream (void* == hipStream_t, NULL = default stream).
 *   - one context per (process, GPU); one host thread per context.
 *   - the engine has NO CPU fallback: creating a context without a usable GPU fails
 *     with RK_ERR_NO_DEVICE.
 */
#ifndef RABBITKSSD_H
#define RABBITKSSD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rk_status {
    RK_OK = 0,
    RK_ERR_ARG = -1,        /* invalid argument (incl. the reference's parameter checks) */
    RK_ERR_NO_DEVICE = -2,  /* no HIP device / device ordinal out of range              */
    RK_ERR_HIP = -3,        /* a HIP runtime call failed                                */
    RK_ERR_NOMEM = -4,      /* host or device allocation failed                         */
    RK_ERR_CAPACITY = -5,   /* caller-provided output buffer too small                  */
    RK_ERR_UNSUPPORTED = -6 /* outside this build's limits (e.g. >= 2^32 postings)      */
} rk_status;

typedef struct rk_ctx rk_ctx;
typedef struct rk_filter rk_filter;
typedef struct rk_sketches rk_sketches;
typedef struct rk_index rk_index;

/* kssd_parameter_t (src/common.h:8-25), the fields the hot path reads. */
typedef struct rk_params {
    int32_t half_k, half_subk, drlevel;
    int32_t rev_add_move, half_outctx_len;
    int32_t dim_start, dim_end;
    uint32_t kmer_size;
    uint64_t domask, tupmask, undomask0, undomask1;
} rk_params;

/* One reported pair.  alldist (triangle=1): row=i, col=j>i, size0=|S_i|, size1=|S_j|
 * (src/dist.cpp:207-217); dist (triangle=0): row=query, col=ref, size0=|ref|,
 * size1=|query| (src/dist.cpp:600-609). */
typedef struct rk_hit {
    uint32_t row, col;
    int32_t common, size0, size1, pad_;
    double jorc; /* jaccard (metric 0) or containment (metric 1) */
    double dist; /* mashD   (metric 0) or AafD        (metric 1) */
} rk_hit;

/* ---- context ------------------------------------------------------------------- */
int rk_device_count(void);
int rk_ctx_create(int device, rk_ctx **out);
/* Objects (rk_filter, rk_sketches, rk_index) must be freed before the context they were created on. */
void rk_ctx_destroy(rk_ctx *ctx);
/* Device memory released by the library's objects and temporaries is cached in the context and handed out
 * again (steady-state calls allocate nothing: hipMalloc/hipFree cost 50-300 us each and hipFree synchronises the
 * device); rk_ctx_trim returns the cached blocks to the driver. */
void rk_ctx_trim(rk_ctx *ctx);
/* out[0] bytes obtained from the driver, out[1] of which idle in the cache, out[2] hipMalloc calls, out[3] hipFree
 * calls made by the context's allocator so far (a steady-state call sequence leaves out[2] and out[3] unchanged). */
void rk_ctx_pool_stats(rk_ctx *ctx, uint64_t out[4]);
/* Measurement: with timing on, a pass brackets its dominant kernel with HIP events on the stream it is launched on;
 * rk_ctx_last_ms(ctx, RK_MS_SKETCH_KERNEL) then returns that kernel's duration in milliseconds for the last
 * rk_sketch_* call.  (The distance entry points launch one kernel per call or band: bracket rk_dist_rows_dev yourself.) */
#define RK_MS_SKETCH_KERNEL 0
/* rk_dist_topn with timing on, summed over its batches: the counting kernel, the selection kernel (its retries included), the
 * candidates' sort + download, the host finish (exact distances + heap); RK_MS_TOPN_CANDIDATES is no time but the number of
 * candidate records the selection kept (0 when the call took the plain path). */
#define RK_MS_TOPN_COUNTS 1
#define RK_MS_TOPN_SELECT 2
#define RK_MS_TOPN_DOWNLOAD 3
#define RK_MS_TOPN_HOST 4
#define RK_MS_TOPN_CANDIDATES 5
/* rk_cluster_rows with timing on: its hook kernel alone (the last hook pass of the call). */
#define RK_MS_CLUSTER_HOOK 6
/* rk_greedy_rows with timing on: all decision rounds of the last call (0 when no record took part). */
#define RK_MS_GREEDY_ROUNDS 7
/* rk_knn_rows with timing on: degree pass through selection kernel of the last call (0 when no record took part or the call
 * took the host path). */
#define RK_MS_KNN_SELECT 8
/* rk_dbscan_rows with timing on: hook kernel through label kernel of the last call (0 when the call took the host path). */
#define RK_MS_DBSCAN 9
/* rk_mreach_rows with timing on: degree pass through the last Boruvka round of the last call (0 when the call took the host path). */
#define RK_MS_MREACH 10
/* rk_medoid_rows with timing on: sums sweep through gather kernel of the last call (0 when the call took the host path). */
#define RK_MS_MEDOID 11
/* rk_assign_rows with timing on: first sweep through gather kernel of the last call (0 when the call took the host path). */
#define RK_MS_ASSIGN 12
void rk_ctx_set_timing(rk_ctx *ctx, int on);
/* A process that makes ONE pass (a command-line tool) says so: the library then keeps work on the host where the device path
 * would first have to load a code object that costs more than it saves on a single call (today: ordering up to 2^18 hit
 * records by (row, col) in rk_dist_rows: 8 ms to load the sort against 3 ms of std::sort for 45,000 records), and a self join
 * never pays for structures that only pay off on later joins.  A context that is NOT single-shot treats an index as resident:
 * from the second unsharded sparse self join over one index on, the tile kernel runs (its records are built by that second
 * call, 1-2 ms once; 0.030 against 0.032 ms per join at 10,000 genomes, 0.084 against 0.115 at 50,000).  Results are the same
 * either way. */
void rk_ctx_set_single_shot(rk_ctx *ctx, int on);
double rk_ctx_last_ms(const rk_ctx *ctx, int which);
const char *rk_last_error(const rk_ctx *ctx);
const char *rk_version(void);
void rk_free_host(void *p);

/* ---- memory / stream helpers ----------------------------------------------------------
 * What a host compiled without the HIP headers (the reference's g++ build) needs to keep the
 * device fed the way src/sketch.cpp's producer/consumer threads keep the CPU cores fed
 * (src/sketch.cpp:318-460): page-locked staging buffers the parser threads fill, device
 * buffers, a stream, and an upload that returns immediately so parsing of the next batch
 * overlaps it.  A stream is an opaque handle; NULL is the default stream. */
int rk_pinned_alloc(rk_ctx *ctx, uint64_t bytes, void **out);
void rk_pinned_free(void *p);
int rk_dev_alloc(rk_ctx *ctx, uint64_t bytes, void **out);
void rk_dev_free(void *p);
int rk_stream_create(rk_ctx *ctx, void **out);
void rk_stream_destroy(void *stream);
int rk_stream_sync(rk_ctx *ctx, void *stream);
int rk_upload_async(rk_ctx *ctx, void *dst_dev, const void *src_host, uint64_t bytes, void *stream);
/* device-to-device copy on `stream` (a host that streams a file of unknown inflated size grows its device buffer) */
int rk_dev_copy_async(rk_ctx *ctx, void *dst_dev, const void *src_dev, uint64_t bytes, void *stream);

/* ---- parameters (host arithmetic only) -------------------------------------------- */
/* RK_ERR_ARG when half_subk - drlevel < 3 (src/common.cpp:37), half_k < half_subk or
 * half_subk >= 8 (src/shuffle.cpp:26,30), half_k > 16. */
int rk_params_init(int half_k, int half_subk, int drlevel, rk_params *out);
/* number of hash bits = 4*(half_k-drlevel); >32 means the 64-bit layout (use64) */
int rk_hash_bits(const rk_params *p);

/* ---- sketching ---------------------------------------------------------------- */
/* Uploads the .shuf table (int32[16^half_subk], src/shuffle.cpp:8-23) and builds the
 * on-chip pre-filter for entries < dim_end. */
int rk_filter_create(rk_ctx *ctx, const rk_params *p, const int32_t *shuffled_dim,
                     rk_filter **out);
void rk_filter_free(rk_filter *f);

/* Sketches n_genomes genomes.  seq holds the sequence bytes of all records back to
 * back (newlines already removed, kseq semantics); rec_off[n_rec+1] delimits records
 * (windows never span records, src/sketch.cpp:487-488); genome_rec[n_genomes+1] gives
 * each genome's record range.  Result: per-genome SORTED UNIQUE 32-bit hashes. */
int rk_sketch_batch(rk_ctx *ctx, const rk_filter *f, const uint8_t *seq, const uint64_t *rec_off,
                    uint64_t n_rec, const uint64_t *genome_rec, uint32_t n_genomes,
                    rk_sketches **out);

/* Same, inputs already packed and resident in HBM: packed_dev holds each genome at
 * gbeg[g] (a multiple of 1024) .. gend[g]; records of a genome are separated by one
 * 0x00 byte and the gap up to the next multiple of 1024 is zero-filled (see
 * rk_pack_layout / rk_pack_genomes).  gbeg/gend are host arrays.  All device work is
 * enqueued on `stream`; the call synchronises that stream before returning (it needs the
 * candidate and hash counts on the host). */
int rk_sketch_packed_dev(rk_ctx *ctx, const rk_filter *f, const uint8_t *packed_dev,
                         uint64_t packed_bytes, const uint64_t *gbeg, const uint64_t *gend,
                         uint32_t n_genomes, void *stream, rk_sketches **out);
/* FASTQ variant of both (sketchFastqFile, src/sketch.cpp:596-890): qual (optional) holds one quality
 * character per base of seq, a base with quality < least_qual is invalid (src/sketch.cpp:785);
 * a hash is kept only if it occurred at least min_count times (leastNumKmer, :828-845).
 * rk_sketch_batch == rk_sketch_batch_ex(qual = NULL, least_qual = 0, min_count = 1). */
int rk_sketch_batch_ex(rk_ctx *ctx, const rk_filter *f, const uint8_t *seq, const uint8_t *qual,
                       int least_qual, uint32_t min_count, const uint64_t *rec_off, uint64_t n_rec,
                       const uint64_t *genome_rec, uint32_t n_genomes, rk_sketches **out);
int rk_sketch_packed_dev_ex(rk_ctx *ctx, const rk_filter *f, const uint8_t *packed_dev,
                            uint64_t packed_bytes, const uint64_t *gbeg, const uint64_t *gend,
                            uint32_t n_genomes, uint32_t min_count, void *stream, rk_sketches **out);
/* Counted variants of the two calls above: the same arguments, the same hashes and offsets byte for byte, and per kept hash
 * the number of candidates (selected k-mer windows) of its genome that carried it -- what the dedup of the uncounted calls
 * computes and drops.  A hash is kept iff its count >= min_count, as above; the count is the full count (>= 1, <= the genome's
 * candidate count), never clipped.  FASTA and FASTQ alike: the quality gate removes windows before they are counted.  The
 * result is an rk_sketches with counts (rk_sketches_has_counts); rk_sketch_last_plan is left as the uncounted calls leave it. */
int rk_sketch_batch_counts(rk_ctx *ctx, const rk_filter *f, const uint8_t *seq, const uint8_t *qual,
                           int least_qual, uint32_t min_count, const uint64_t *rec_off, uint64_t n_rec,
                           const uint64_t *genome_rec, uint32_t n_genomes, rk_sketches **out);
int rk_sketch_packed_dev_counts(rk_ctx *ctx, const rk_filter *f, const uint8_t *packed_dev,
                                uint64_t packed_bytes, const uint64_t *gbeg, const uint64_t *gend,
                                uint32_t n_genomes, uint32_t min_count, void *stream, rk_sketches **out);
/* What the last rk_sketch_packed_dev(_ex) call on this context did (rk_sketch_batch(_ex) end in one): the scan kernel as a
 * profiler prints it (e.g. "rk_scan2_kernel<20, 8>", "rk_sketch_kernel<0, 0, false, 1>"), the LDS image (2 two-stage scan,
 * 1 / 0 rk_sketch_kernel with the 64 / 144 KiB image) and whether the exact table confirms the survivors, the chunk length in
 * 1 KiB blocks, the chunks, the workgroups launched and the ticket groups they draw from, the passes taken (2: a candidate
 * region overflowed and the pass ran again with exact capacities), and of the last pass: the genomes sorted device-wide (region
 * beyond the LDS sort), the largest candidate count and the largest region capacity of a genome.  Every field is host
 * arithmetic of the call or comes home in its one read-back: the record costs no launch and no copy.  A call that scanned
 * nothing (no chunks) leaves kernel empty and grid 0.  RK_ERR_ARG for null pointers, RK_ERR_UNSUPPORTED before the first call. */
typedef struct rk_sketch_plan {
    char kernel[64];
    int32_t image, exact;
    uint32_t chunk_blocks, n_chunks, grid, n_groups;
    uint32_t attempts, n_big;
    uint32_t max_candidates, max_reg_cap;
} rk_sketch_plan;
int rk_sketch_last_plan(const rk_ctx *ctx, rk_sketch_plan *out);
/* host helpers for the packed layout: sizes first, then fill a caller buffer */
int rk_pack_layout(const uint64_t *rec_off, uint64_t n_rec, const uint64_t *genome_rec,
                   uint32_t n_genomes, uint64_t *gbeg, uint64_t *gend, uint64_t *packed_bytes);
int rk_pack_genomes(const uint8_t *seq, const uint64_t *rec_off, uint64_t n_rec,
                    const uint64_t *genome_rec, uint32_t n_genomes, const uint64_t *gbeg,
                    uint8_t *packed, uint64_t packed_bytes);

/* device-resident CSR of sketches.  A genome's hashes may come in any order (the reference writes `unordered_set`
 * iteration order, src/sketch.cpp:537-553): the library sorts them on the device, rk_sketches_download returns them
 * ascending.  A sketch that repeats a hash keeps its repeats (they count, src/dist.cpp:199-202). */
int rk_sketches_from_host(rk_ctx *ctx, const uint32_t *hashes, const uint64_t *off,
                          uint32_t n_genomes, rk_sketches **out);
/* same from device-resident arrays (copied device-to-device into a library-owned object).  The copies run on the
 * context's own stream: the arrays must be COMPLETE when the call is made (synchronise the stream that produced them
 * first).  RK_ERR_ARG when off_dev is not a CSR offset table (off[0] = 0, non-decreasing). */
int rk_sketches_from_dev(rk_ctx *ctx, const uint32_t *hashes_dev, const uint64_t *off_dev,
                         uint32_t n_genomes, rk_sketches **out);
/* 64-bit hash layout (use64: half_k - drlevel > 8, src/sketch.cpp:336): the sketch kernel produces it
 * by itself when rk_hash_bits() > 32; these move such sketches across the boundary. */
int rk_sketches_from_host64(rk_ctx *ctx, const uint64_t *hashes, const uint64_t *off,
                            uint32_t n_genomes, rk_sketches **out);
int rk_sketches_download64(const rk_sketches *s, uint64_t *hashes, uint64_t *off);
int rk_sketches_is64(const rk_sketches *s);
uint32_t rk_sketches_count(const rk_sketches *s);
uint64_t rk_sketches_total(const rk_sketches *s);
/* number of k-mer windows seen by the last sketch call that produced s (0 if imported) */
uint64_t rk_sketches_windows(const rk_sketches *s);
/* copies off[n+1] and hashes[total] to caller buffers (either may be NULL) */
int rk_sketches_download(const rk_sketches *s, uint32_t *hashes, uint64_t *off);
const uint32_t *rk_sketches_hashes_dev(const rk_sketches *s);
const uint64_t *rk_sketches_off_dev(const rk_sketches *s);
/* Counted sketches.  An rk_sketches may carry an optional device array counts[total], aligned with its hashes: counts[i] is the
 * multiplicity of hash i in its genome.  The counted sketch calls produce it, rk_sketches_from_host_counts imports it.
 * Every consumer of sketches but two ignores the counts -- rk_index_build, the joins (rk_dist_rows, rk_dist_topn, ...), rk_sketches_mask,
 * rk_group_sketches, rk_gather_rows, rk_screen_rows, rk_lca_rows, the shard calls -- and the objects they derive carry none.  The two
 * that read them: rk_screen_abund_rows, the screen with the median and the summed multiplicity of every record, and
 * rk_sketches_mask_counts, whose survivors keep their counts.
 *   rk_sketches_has_counts       1 with counts, 0 without (or s == NULL)
 *   rk_sketches_counts_dev       the device array, NULL without counts
 *   rk_sketches_download_counts  copies counts[total] to a caller buffer; RK_ERR_UNSUPPORTED without counts
 *   rk_sketches_from_host_counts imports hashes (uint32_t[total], or uint64_t[total] when wide != 0), counts and offsets.  Every
 *                                genome's hashes must be strictly ascending -- the library sorts uncounted imports, which would tear
 *                                the counts from their hashes -- and every count at least 1: RK_ERR_ARG otherwise (checked on the
 *                                device; nothing is created). */
int rk_sketches_has_counts(const rk_sketches *s);
const uint32_t *rk_sketches_counts_dev(const rk_sketches *s);
int rk_sketches_download_counts(const rk_sketches *s, uint32_t *counts);
int rk_sketches_from_host_counts(rk_ctx *ctx, const void *hashes, int wide, const uint32_t *counts, const uint64_t *off,
                                 uint32_t n_genomes, rk_sketches **out);
void rk_sketches_free(rk_sketches *s);

/* ---- inverted index ------------------------------------------------------------- */
/* Builds the reference index from device-resident sketches: postings ordered
 * (hash asc, genome asc) exactly like the .dict file, a compact CSR over the distinct
 * hashes, and the per-hash "later genomes" ranges used by the all-vs-all triangle. */
int rk_index_build(rk_ctx *ctx, const rk_sketches *s, int hash_bits, rk_index **out);
/* From the on-disk pair: postings = .dict payload (u32[total]), counts = the dense
 * u32[2^hash_bits] array of the .index file, ref_sizes = sketch sizes of the
 * reference genomes (from the .sketch).  Replaces the load + prefix sum of
 * src/dist.cpp:86-129. */
int rk_index_import(rk_ctx *ctx, const uint32_t *postings, uint64_t total, const uint32_t *counts,
                    int hash_bits, const uint32_t *ref_sizes, uint32_t n_ref, rk_index **out);
/* To the on-disk pair: postings[total] and (optional) dense counts[2^hash_bits]. */
int rk_index_export(const rk_index *idx, uint32_t *postings, uint32_t *counts);
/* The same content without the dense array: the distinct hashes (ascending, rk_index_distinct() of them) and the length of
 * each one's posting list -- 8 bytes per distinct hash instead of 4 * 2^hash_bits; a host that writes the dense .index
 * file (src/sketch.cpp:1008-1011) scatters the counts into the zero-filled file itself.  32-bit hash layout only. */
int rk_index_export_lists(const rk_index *idx, uint32_t *postings, uint32_t *hashes, uint32_t *counts);
/* 64-bit hash layout: the sparse .index variant {u64 n; u64 hash[n]; u32 count[n]} with the .dict
 * posting blocks in the same order (src/sketch.cpp:942-963, read at src/dist.cpp:36-82).  Export
 * lists the hashes ascending; import accepts any block order (the reference writes hash-map order). */
int rk_index_export64(const rk_index *idx, uint32_t *postings, uint64_t *hashes, uint32_t *counts);
int rk_index_import64(rk_ctx *ctx, const uint32_t *postings, uint64_t total, const uint64_t *hashes,
                      const uint32_t *counts, uint64_t n_hash, int hash_bits, const uint32_t *ref_sizes,
                      uint32_t n_ref, rk_index **out);
/* Internal genome order.  rk_index_build renumbers the genomes so that relatives (genomes that share several of their
 * smallest hashes) become neighbours, whatever order the collection was listed in -- the reference's OpenMP loop leaves
 * them in completion order (src/sketch.cpp:558-568); the device layout (compact posting slices, row pairs) relies on
 * neighbours being relatives.  Nothing of this is visible in results: hit records, dense counter rows and exported
 * postings carry the caller's genome indices.  It only decides WHICH pairs a row shard (rk_dist_opts.row_first/row_step/
 * row_block) computes: shards partition the rows of the internal order.  orig_out[i] = caller's index of internal genome i. */
int rk_index_order(const rk_index *idx, uint32_t *orig_out);
uint64_t rk_index_total(const rk_index *idx);    /* H = number of postings        */
uint64_t rk_index_distinct(const rk_index *idx); /* U = number of distinct hashes */
uint32_t rk_index_genomes(const rk_index *idx);
int rk_index_hash_bits(const rk_index *idx);
/* 1 when rk_index_build took its bucket-sort path (set sketches with 32-bit hashes whose buckets fit the LDS sort),
 * 0 for the general path (device-wide radix sort) or an imported index: lets a harness say which build it timed. */
int rk_index_built_fast(const rk_index *idx);
/* Which build rk_index_build / rk_index_build_shard WOULD run for these sketches, under the developer switches of the context
 * and of the environment as they are now: the knobs, the build's plan and the plan of its first bucket-sort attempt -- host
 * arithmetic alone, nothing is launched or allocated.  Returns what the plan returns (its refusals included: out[] is then
 * untouched) and writes RK_PLAN_WORDS words.  A build may still end elsewhere -- its kernels raise flags, attempts are
 * repeated --: rk_index_build_report says how it did end.  For tests and harnesses (which kernels did I time?). */
enum {
    RK_PLAN_FAST_OK = 0,   /* the bucket sort is tried at all (else: the general path, a device-wide radix sort)        */
    RK_PLAN_TILES_MODE,    /* its first attempt emits tile records (else slice records)                                 */
    RK_PLAN_SLICES_OK,     /* the key fields and sizes admit slice records                                              */
    RK_PLAN_TILES_OK,      /* ... tile records                                                                          */
    RK_PLAN_B,             /* bucket bits                                                                               */
    RK_PLAN_LOW_BITS,      /* hash bits below the bucket                                                                */
    RK_PLAN_GB,            /* genome bits of a key                                                                      */
    RK_PLAN_RB,            /* position bits of a key (slice records)                                                    */
    RK_PLAN_N_PASS,        /* range passes over the hash space                                                          */
    RK_PLAN_RANGE_BITS,    /* top hash bits that select a range (shards and passes)                                     */
    RK_PLAN_PART2,         /* the two-pass partition (coarse + fine) instead of the one scattering pass                 */
    RK_PLAN_USE_FILTER,    /* a range pass partitions a filtered copy of its hashes                                     */
    RK_PLAN_SMALL_WGS,     /* the coarse pass in four workgroups of 256 threads per chunk (else one of 1,024)           */
    RK_PLAN_NARROW,        /* (hash_low, genome) sort keys of 32 bits (else 64)                                         */
    RK_PLAN_BIG_OK,        /* buckets beyond the in-LDS sort are built slab by slab instead of refusing the bucket sort */
    RK_PLAN_RELABEL,       /* the genomes are renumbered (rk_index_order)                                               */
    RK_PLAN_TWO_STREAMS,   /* ... on a stream of its own                                                                */
    RK_PLAN_EMIT_T,        /* threads per bucket of the emission, as dispatched: 256, 512 or 1024                       */
    RK_PLAN_KEYS_CAP,      /* keys the buffers of a pass hold                                                           */
    RK_PLAN_REC_CAP,       /* unsorted tile records the first attempt has room for (0: slice records)                   */
    RK_PLAN_WORDS
};
int rk_index_build_plan(rk_ctx *ctx, const rk_sketches *sketches, int hash_bits, uint32_t shard, uint32_t n_shards, int64_t out[]);
/* How the build of this index ended: all zeros for an index that was imported, unpacked, broadcast or joined from a shard's
 * records.  Host bookkeeping of rk_index_build, no device work. */
enum {
    RK_REPORT_ATTEMPTS = 0,  /* attempts of the bucket sort (0: the plan went straight to the general path)              */
    RK_REPORT_KEY_RETRIES,   /* of which repeated because a range pass held more keys than its buffers                   */
    RK_REPORT_REC_RETRIES,   /* ... because the tile records did not fit                                                 */
    RK_REPORT_FELL_BACK,     /* 1: tile records were given up for slice records                                          */
    RK_REPORT_GENERAL,       /* 1: the general path built the index                                                      */
    RK_REPORT_FLAGS,         /* what the kernels of the last attempt raised: 1 a bucket or a pass beyond its buffer, 2 a
                                hash outside the hash space                                                              */
    RK_REPORT_HEAVY,         /* buckets the last attempt left to the slab-by-slab kernel, summed over its passes         */
    RK_REPORT_PASSES,        /* passes of the last attempt                                                               */
    RK_REPORT_WORDS
};
int rk_index_build_report(const rk_index *idx, uint64_t out[8]);
/* Which structures of the all-vs-all join the index carries right now, as a bit mask: 1 = slice records (one per (genome,
 * hash) element: rk_near_kernel, rk_dist_kernel), 2 = tile records (one per posting list and pair of 32-genome blocks it
 * touches: rk_tile_kernel), 4 = the tile records came with rk_index_build itself (collections of RK_DIST_TILES_MIN_GENOMES =
 * 4,000 genomes and more: the FIRST self join already runs on the tile kernel; slice records are then made on first use --
 * a dense report, RK_DIST_TILES=0).  Which kernel a self join takes depends on this, the index's size and the options --
 * never on how often the index was joined before.  (The reference has one loop for every collection, src/dist.cpp:174-258.) */
int rk_index_products(const rk_index *idx);
/* sum over all reference hashes h of c_h^2 = postings streamed by a full alldist
 * (the T of the roofline formula) */
uint64_t rk_index_sum_sq(const rk_index *idx);
/* The all-vs-all join reads one 8-byte slice record per (genome, hash) pair with later sharers.  out[0] = records,
 * out[1] = of which in compact form (first genome + bitmask: the record IS the posting list, no posting is gathered),
 * out[2] = records the row-pair kernel walks (the rest are covered by the pair partner), out[3] = the 8-byte tile records of
 * the tile kernel (one per posting list and pair of 32-genome blocks it touches; 0 while the index has none: rk_index_products).
 * Computed on first request (one small kernel) and cached; 0s for an imported index. */
int rk_index_self_stats(const rk_index *idx, uint64_t out[4]);
/* Multi-GPU, sharded build (round 5).  The all-vs-all join shards twice: the BUILD by hash range (a posting list lives in one
 * range: its tile records are found without looking at the other ranges), the JOIN by rows (a tile of the pair matrix belongs
 * to the shard of its row block; blocks of 32 genomes of the internal order dealt round-robin, as rk_dist_opts.row_block = 32
 * does).  Between the two lies ONE all-to-all of 12-byte tile records -- no index is replicated, nothing is reduced:
 *   every shard:  rk_index_build_shard(sketches, hash_bits, shard, n_shards)   the lists of hash range `shard` (n_shards a power of
 *                 two <= 64; every shard holds the same CSR sketches -- one broadcast -- and computes the same internal order)
 *                 rk_index_shard_records(part, counts[n_shards])    tile records it holds for every destination shard
 *                 rk_index_shard_pack(part, send_dev, stream)       ... contiguous by destination (12 bytes each)
 *   (the caller's all-to-all: RCCL / torch.distributed.all_to_all_single, or peer copies)
 *                 rk_index_join_shard(ctx, part, recv_dev, n, &join)  sorts what arrived by tile: a join-only index over THIS
 *                 shard's rows; rk_dist_rows(_dev)(join, NULL, opts with row_step = 1) reports the pairs whose row block it
 *                 owns.  The union over the shards is the whole result (the reference's rows are independent, src/dist.cpp:174).
 * A collection too big for one pass of the bucket sort (more than ~5 * 10^7 postings) is built the same way on ONE device:
 * rk_index_build covers the hash space range by range, the postings of a range behind those of the range before. */
int rk_index_build_shard(rk_ctx *ctx, const rk_sketches *s, int hash_bits, uint32_t shard, uint32_t n_shards, rk_index **out);
int rk_index_shard_records(const rk_index *part, uint64_t *counts_out);
int rk_index_shard_pack(const rk_index *part, void *send_dev, void *stream);
int rk_index_join_shard(rk_ctx *ctx, const rk_index *part, const void *recv_dev, uint64_t n_records, rk_index **out);
/* One process, one context per GPU (`rabbit_kssd alldist --gpus N`): the exchange without a communicator -- GPU d pulls chunk d
 * of every shard's packed records over its own links (hipMemcpyPeerAsync, bounded wait).  parts[r] = shard r of n, each on its own
 * context; recv_dev[d] (free with rk_dev_free) and n_recv[d] are what rk_index_join_shard takes on GPU d.
 * Called from one host thread; the shard builds before it and the joins behind it may run one thread per GPU. */
int rk_index_shard_exchange(rk_index *const *parts, uint32_t n, void **recv_dev, uint64_t *n_recv);
/* The same sharded build from PER-RANK sketches.  A collection sketched on N ranks (the reference's per-genome loop shards by
 * genome with no communication, src/sketch.cpp:455) is not replicated: rank r holds the genomes genome_base .. genome_base +
 * rk_sketches_count(local) - 1 of a collection of n_genomes (contiguous ranges in rank order; every rank holds at least one genome).
 * Instead of broadcasting the collection, every rank cuts its sketches into keys by destination shard, ONE all-to-all moves them,
 * and every shard builds its posting lists from the keys that arrived:
 *   every rank:   rk_sketches_signature(local, sig_dev)           68 bytes per genome, all-gathered (the renumbering reads them)
 *                 rk_sketches_shard_keys(local, ..., counts)       keys for every destination shard
 *                 rk_sketches_shard_pack(local, ..., send_dev)     ... contiguous by destination (8 bytes each)
 *   (the caller's all-to-all of the keys)
 *   every shard:  rk_index_build_shard_keys(keys, n, sig, ...)     a shard index like rk_index_build_shard's: the same rk_index_order,
 *                 rk_index_total and rk_index_shard_records; rk_index_shard_pack / rk_index_join_shard / rk_dist_rows as above.
 * Signature: sig_dev[g * RK_SIG_WORDS] = size of local genome g, then its min(16, size) smallest hashes ascending (64-bit hashes folded
 * to 32 bits as hash ^ hash >> 32, the fold of the renumbering), zero-padded.  Asynchronous on `stream`.
 * Wire format of a key (u64): (hash & (2^(hash_bits - shard_bits) - 1)) << gb | global genome id, where shard_bits = log2(n_shards),
 * gb = the smallest gb >= 1 with 2^gb >= n_genomes, and the destination shard of the key is hash >> (hash_bits - shard_bits).
 * RK_ERR_ARG: n_shards not a power of two up to 64, genome_base + rk_sketches_count(local) > n_genomes, an empty `local`, a hash
 * beyond hash_bits (rk_sketches_shard_keys; the pack leaves such hashes out).  RK_ERR_UNSUPPORTED: local sketches that are not sets
 * (a genome lists a hash twice), a key that does not fit 64 bits (hash_bits - shard_bits + gb > 64).
 * rk_sketches_shard_pack enqueues on `stream` and returns without waiting.
 * rk_index_build_shard_keys takes the keys that arrived (any order, any source; the buffer is read, never written) and the
 * all-gathered signatures of all n_genomes (n_genomes * RK_SIG_WORDS u32, in global genome order); 2 .. 64 shards.  Its arrays that
 * scale with postings are sized by the keys of the shard, not by the collection.  RK_ERR_ARG for a key outside the wire format (hash
 * bits beyond hash_bits - shard_bits, a genome id >= n_genomes): the build is refused, no key is dropped or cut down.
 * RK_ERR_UNSUPPORTED, besides rk_index_build_shard's own limits, when fewer than 7 hash bits remain inside a shard (hash_bits -
 * shard_bits < 7, or fewer inside one of its passes): the keys are partitioned by the two-pass bucket sort, which needs >= 128
 * buckets (rk_index_build_shard builds such tiny hash spaces another way, from the sketches). */
#define RK_SIG_WORDS 17
int rk_sketches_signature(rk_ctx *ctx, const rk_sketches *local, void *sig_dev, void *stream);
int rk_sketches_shard_keys(rk_ctx *ctx, const rk_sketches *local, uint32_t genome_base, uint32_t n_genomes, int hash_bits,
                           uint32_t n_shards, uint64_t *counts_out);
int rk_sketches_shard_pack(rk_ctx *ctx, const rk_sketches *local, uint32_t genome_base, uint32_t n_genomes, int hash_bits,
                           uint32_t n_shards, void *send_dev, void *stream);
int rk_index_build_shard_keys(rk_ctx *ctx, const void *keys_dev, uint64_t n_keys, const void *sig_dev, uint32_t n_genomes,
                              int hash_bits, uint32_t shard, uint32_t n_shards, rk_index **out);
/* Multi-GPU: the whole index as ONE contiguous device blob, so that the owner can hand it
 * to an RCCL broadcast (one collective, no reduction: query rows are independent) and every
 * peer rebuilds an identical rk_index from the received bytes.  pack/unpack only enqueue
 * device-to-device copies on `stream` and synchronise it before returning. */
uint64_t rk_index_blob_bytes(const rk_index *idx);
int rk_index_pack_dev(const rk_index *idx, void *blob_dev, uint64_t blob_cap, void *stream);
int rk_index_unpack_dev(rk_ctx *ctx, const void *blob_dev, uint64_t blob_bytes, void *stream,
                        rk_index **out);
/* The same inside ONE process that drives several GPUs (one context and one host thread per GPU): replicates the
 * index of src's context onto each of the n_dst contexts, all peers copying at the same time over their own xGMI link
 * (hipMemcpyPeerAsync; contexts on the source's device get a device-to-device copy).  out[i] belongs to dst[i]. */
int rk_index_broadcast(const rk_index *src, rk_ctx *const *dst, uint32_t n_dst, rk_index **out);
void rk_index_free(rk_index *idx);

/* ---- distances ------------------------------------------------------------------- */
typedef struct rk_dist_opts {
    int32_t triangle;   /* 1: alldist (queries ARE the indexed sketches, cols j>i, keep
                              dist <  max_dist, src/dist.cpp:207,232)
                           0: dist (all cols, keep dist <= max_dist, src/dist.cpp:600,624) */
    int32_t metric;     /* 0 jaccard->mashD, 1 containment->AafD (-M)                  */
    int32_t kmer_size;  /* 2*half_k                                                    */
    int32_t row_block;  /* rows are dealt to the shards in blocks of row_block consecutive rows
                           (block-cyclic); 0,1 = single rows.  An even row_block lets the
                           all-vs-all kernel walk neighbouring rows in pairs, a multiple of 32
                           lets the tile kernel count every tile on one shard only (32 is a
                           good value for multi-GPU runs)                                   */
    double max_dist;    /* -D                                                          */
    uint32_t row_first; /* this shard owns blocks row_first, row_first+row_step, ...:  */
    uint32_t row_step;  /*   row sharding across GPUs; 0,1 = all rows.  queries == NULL (self join): rows of the
                             index's internal genome order (rk_index_order); a reported pair belongs to the shard of
                             its member that comes first in that order                                            */
} rk_dist_opts;

/* The tile kernel is output-sensitive: of the 32 x 32 tiles of the pair matrix that hold a record at all, a launch gives a
 * workgroup only to those that can hold a reportable pair under `opts` (records per smallest sketch of the tile against the
 * threshold; the test is exact, the counted tiles are counted exactly).  out[0] = tiles with records, out[1] = tiles a launch
 * with these options starts (opts == NULL: 0), out[2] = tile records, out[3] = record slots (every tile from an even slot).
 * All 0 while the index has no tile records.  (The reference forms every cell of every row, src/dist.cpp:194-255.) */
int rk_index_tile_stats(const rk_index *idx, const rk_dist_opts *opts, uint64_t out[4]);

/* Counts |S_q n S_r| through the inverted index and applies the reference's epilogue.
 * queries == NULL is only valid with triangle=1 (the indexed sketches are the queries).
 * hits_out is library-allocated (rk_free_host), sorted by (row, col).  The jaccard/containment and
 * distance of every returned pair are recomputed on the host with the C library's log -- the
 * expression of src/dist.cpp:218-231 / :239-252 -- and the threshold is applied to that value (the
 * device reports with a threshold a few ulps wider): values and hit set are the reference's bit for bit.
 * common_dense (optional, host, n_query*n_ref int32, row-major) receives the full
 * counter rows of the selected rows (other rows untouched) -- used by parity tests. */
int rk_dist_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries,
                 const rk_dist_opts *opts, rk_hit **hits_out, uint64_t *n_hits,
                 int32_t *common_dense);

/* Asynchronous all-in-HBM variant: hits are appended (unordered) to hits_dev
 * (capacity hits_cap records); *n_hits_dev (uint64, zeroed by the caller) counts every
 * hit, including those beyond the capacity, so an overflow is detectable.  Distances here are the
 * device's own FP64 evaluation (its log may differ from the C library's in the last bit: <= 1e-12).
 * Concurrency: calls with explicit queries and self joins that run on the tile kernel (collections with wide clusters or
 * tiny sketches, RK_DIST_TILES=1) keep no per-launch state in the index and may overlap freely on different streams.  A
 * self join that runs on the near-window kernel keeps its fallback list IN the index: at most one such self join per index
 * may be in flight at a time (serialise them on one stream, or use one index object per stream).  (With RK_DISTQ_SLICED=1 --
 * a measured, slower variant of the query path, off by default -- the scratch of the membership pass is kept with the QUERY
 * sketches: one call per query-sketches object at a time.)
 * Limits: fewer than 2^31-1 genomes and 2^32-1 postings per index.  From 2^31-1 postings on (all of GenBank's bacteria at
 * ~1,200 hashes each) rk_index_build leaves out the slice records of the row kernels (their posting offsets would collide
 * with the tag bit of the compact form): export, explicit queries below 2^31 postings and SPARSE self joins (the tile
 * kernel reads the posting lists themselves) work on such an index; a dense self join (a threshold that admits distance
 * 1.0) and sketches that repeat a hash return RK_ERR_UNSUPPORTED. */
int rk_dist_rows_dev(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries,
                     const rk_dist_opts *opts, rk_hit *hits_dev, uint64_t hits_cap,
                     uint64_t *n_hits_dev, void *stream);

/* Name (as a profiler prints it, e.g. "rk_dist_kernel<true, 2, 512>") of the kernel rk_dist_rows(_dev) launches for
 * these arguments: lets a harness check that a stored counter profile belongs to the variant it is timing.  A big self
 * join runs as several launches (bands of rows, each with LDS rows as wide as the columns behind its first row): the
 * name is then that of the first band followed by " [N bands]". */
int rk_dist_kernel_name(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_dist_opts *opts,
                        char *buf, size_t cap);

/* -N: keeps, per query row, the max_neighbor nearest hits with the reference's heap
 * order (emitted largest distance first).  hits must be sorted by (row, col); the
 * result is written in place and its length returned through n_hits. */
int rk_topn_rows(rk_hit *hits, uint64_t *n_hits, uint64_t max_neighbor);

/* -N on the device: per selected query row, the max_neighbor nearest references under opts (triangle must be 0;
 * row_first/row_step/row_block as in rk_dist_rows).  Returns exactly the records, values and order of
 * rk_dist_rows(...) followed by rk_topn_rows(..., max_neighbor): rows ascending, within a row the reference heap's
 * pop order (largest distance first).  Device and host memory are O(batch + Q * max_neighbor), never O(Q * R): a batch
 * of query rows is counted into int32 counter rows, a selection kernel keeps per row only the cells that can reach the
 * reference's heap (room for min(R, 1024 + 16 * max_neighbor) per row), and the host replays that heap over them.  Counter
 * rows and candidate buffers of a batch fit RK_TOPN_BATCH_BYTES (default 1 GiB; at least one row); a row with more
 * candidates than its room grows the buffer to the exact count, never beyond the batch's rows x R.
 * Thresholds that exclude distance 1.0 (their output is bounded by the hits anyway), max_neighbor above 1,024 and
 * RK_DIST_TOPN=0 run as rk_dist_rows + rk_topn_rows inside the call.  max_neighbor == 0 returns no record and runs nothing
 * on the device.  RK_ERR_ARG for triangle == 1 (the reference has no -N for alldist) and null pointers.
 * hits_out: library-allocated (rk_free_host). */
int rk_dist_topn(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_dist_opts *opts,
                 uint64_t max_neighbor, rk_hit **hits_out, uint64_t *n_hits);

/* ---- clusters --------------------------------------------------------------------- */
/* Single-linkage clusters of the all-vs-all: the connected components of the graph whose edges are the pairs
 * rk_dist_rows(ctx, idx, NULL, opts, ...) would report -- same metric, same strict threshold (dist < max_dist decided with the C
 * library's log, src/dist.cpp:232), same row_first / row_step / row_block selection, any index that call accepts (the join-only
 * index of rk_index_join_shard included).  labels_out[i] (host, rk_index_genomes(idx) entries, caller's genome order) = the
 * SMALLEST caller index of i's component: labels_out[labels_out[i]] == labels_out[i] and labels_out[i] <= i.  The result does
 * not depend on the order of hits, genomes or shards.
 * The hit records never leave the device: the self join (rk_dist_rows_dev, threshold widened by 2^-46 as rk_dist_rows widens
 * it) appends them to a device buffer of max(65,536, rows * 64) records (on overflow the join runs again with the exact count),
 * a lock-free union-find links them in one pass, a second kernel writes the labels.  A record whose device distance lies within
 * 2^-46 relative of the threshold is not linked on the device: it goes to a small buffer (4,096 records, RK_CLUSTER_EDGE_CAP; on
 * overflow the linking pass alone runs again with the exact count), the host decides it with the C library's log and unites it
 * into the labels.  PCIe traffic: 4 * N bytes of labels, the borderline records (20 bytes each, usually none) and two counters
 * -- never O(hits); nothing is sorted.
 * A dense report (a threshold above 1.0: every pair is a hit) is answered on the host from the row selection, without a join:
 * all labels 0 for the whole collection; a row shard links its first row to every later genome of the internal order.
 * -D within 2^-46 of 1.0 from below: the widening stops at 1.0 (beyond it the join would turn to the dense report).
 * RK_ERR_ARG: triangle != 1, null pointers, an index rk_dist_rows refuses for a self join (imported, or one hash range of a
 * sharded build).  RK_ERR_UNSUPPORTED comes from the join (rk_dist_rows_dev).  An index without genomes: RK_OK, nothing runs.
 * stats is optional. */
typedef struct rk_cluster_stats {
    uint64_t edges;          /* hit records the hook pass consumed */
    uint64_t borderline;     /* of which sent to the host */
    uint64_t borderline_kept;
    uint32_t join_attempts;  /* 2: the hit buffer overflowed once */
    uint32_t hook_attempts;  /* 2: the borderline buffer overflowed once */
    uint32_t n_clusters;     /* components, singletons included */
    uint32_t pad_;
} rk_cluster_stats;
int rk_cluster_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, uint32_t *labels_out /* host, N */,
                    rk_cluster_stats *stats /* optional */);
/* Host only: the components of the union of two partitions of n genomes, both given as label arrays of the form above, written
 * in the same form -- what folds the labels of row shards and of GPUs into those of the collection.  out may alias a.
 * RK_ERR_ARG for an entry >= n or null pointers. */
int rk_cluster_merge(const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *out);

/* Minimum spanning forest of the all-vs-all: the single-linkage dendrogram up to -D.  The graph is that of rk_cluster_rows (the pairs
 * rk_dist_rows(ctx, idx, NULL, opts, ...) would report: same metric, same strict threshold, same row selection, any index that call
 * accepts, the join-only index of rk_index_join_shard included); an edge is one hit record.
 * Order of edges: the ratio common / u descending (nearest pair first), then row ascending, then col ascending -- u = size0 + size1
 * - common for metric 0, min(size0, size1) for metric 1: both distances fall strictly as the ratio rises, so no log orders edges.
 * Ratios are compared exactly (25/75 and 20/60 tie: row and col decide).  The order is strict, so the forest is unique: the edges
 * Kruskal accepts in this order.  edges_out (library-allocated, rk_free_host; at most rk_index_genomes(idx) - 1 records) lists them in
 * this order; their jorc and dist are recomputed on the host with the C library's log, as rk_dist_rows does: the reference's values
 * bit for bit.  Cut at any t <= max_dist (rk_forest_cut) the forest gives the labels rk_cluster_rows returns at t -- assuming only
 * that the C library's log is monotone over the ratios that occur.  The result does not depend on the order of hits, genomes or
 * shards.
 * The hit records never leave the device (the frame of rk_cluster_rows: the join through rk_dist_rows_dev with the threshold widened
 * by 2^-46 into max(65,536, rows * 64) records, once more with the exact count on overflow).  Boruvka rounds run over them: per round
 * every component finds its best edge (a 64-bit atomic minimum on the weight key ~floor(common * 2^62 / u), then on row << 32 | col
 * among the records that match it), the chosen records are appended to the forest buffer and their components united by the
 * compare-and-swap hook of rk_cluster_rows; the host reads one counter per round and stops at the first round that appended nothing
 * (at most 2 + ceil(log2 N) rounds).  The forest records are sorted on the device and downloaded: 40 bytes per edge, never O(hits).
 * A record whose device distance lies within 2^-46 relative of the threshold (borderline), and a record outside 0 < common <= u (only
 * sketches that repeat hashes have such), takes no part on the device: it goes to the small host buffer of rk_cluster_rows (4,096
 * records, RK_CLUSTER_EDGE_CAP; on overflow that pass alone runs again), the host decides it with the C library's log and folds the
 * kept ones in with a Kruskal over (forest + kept) -- MSF(E1 + E2) = MSF(MSF(E1) + E2).
 * RK_ERR_ARG: triangle != 1, null pointers, a dense report (a threshold above 1.0: a forest over pairs that share nothing is not
 * offered), an index rk_dist_rows refuses for a self join.  RK_ERR_UNSUPPORTED: a sketch of 2^30 hashes or more (the key), and what
 * the join answers.  An index without genomes: RK_OK, no edge, *edges_out = NULL.  stats is optional. */
typedef struct rk_forest_stats {
    uint64_t edges;          /* hit records of the join */
    uint64_t borderline;     /* of which sent to the host */
    uint64_t borderline_kept;
    uint32_t join_attempts;  /* 2: the hit buffer overflowed once */
    uint32_t border_attempts; /* 2: the host buffer overflowed once */
    uint32_t rounds;         /* Boruvka rounds, the last (empty) one included; 0 when no record took part */
    uint32_t n_trees;        /* genomes minus returned edges: components, singletons included */
} rk_forest_stats;
int rk_forest_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, rk_hit **edges_out, uint64_t *n_edges,
                   rk_forest_stats *stats /* optional */);
/* Host only: the forest of the union of two edge lists over n genomes (Kruskal in the order above; `metric` as rk_dist_opts.metric) --
 * what folds the forests of row shards and of GPUs into that of the collection.  The lists need not be forests nor in order.  out is
 * library-allocated (rk_free_host), in order.  RK_ERR_ARG for an edge that names a genome >= n or null pointers (a list of no edges
 * may be NULL). */
int rk_forest_merge(const rk_hit *a, uint64_t na, const rk_hit *b, uint64_t nb, uint32_t n, int metric, rk_hit **out, uint64_t *n_out);
/* Host only: the labels of the forest cut at max_dist, in the form of rk_cluster_rows (labels_out[i] = the smallest index of i's
 * component): an edge links iff its stored dist < max_dist.  RK_ERR_ARG for an edge that names a genome >= n or null pointers. */
int rk_forest_cut(const rk_hit *edges, uint64_t n_edges, uint32_t n, double max_dist, uint32_t *labels_out /* n */);

/* ---- greedy representatives ------------------------------------------------------- */
/* Greedy incremental clustering of the all-vs-all (the rule of CD-HIT and of clust-greedy in RabbitTClust): one representative per
 * group of near genomes -- the list a dereplication feeds to its next `dist` run.  The graph is that of rk_cluster_rows for ALL rows:
 * the pairs rk_dist_rows(ctx, idx, NULL, opts, ...) would report, same metric, same strict threshold decided with the C library's log.
 * Genome a PRECEDES b iff (priority[a], a) < (priority[b], b); with priority == NULL the larger sketch comes first, then the smaller
 * caller index: (-size[a], a) with the sizes the index holds.  Walking the genomes in this order, a genome is a representative iff no
 * representative that precedes it is adjacent to it; every other genome is a member of the NEAREST adjacent representative that
 * precedes it (a nearer one that comes later is not considered, as in the sequential loop).  Nearest: the largest ratio common / u in
 * the exact order of rk_forest_rows (25/75 ties 20/60); ties go to the representative with the smallest caller index.  The result is
 * unique: it does not depend on the order of hits, the internal genome order or the kernel the join took.  Representatives are
 * pairwise not adjacent, and every member is adjacent to its own.
 * rep_out[i] (host, rk_index_genomes(idx) entries) = the caller index of i's representative, i itself iff i is one.  links_out
 * (library-allocated, rk_free_host; NULL when there is none) holds one record per member, by the member's caller index ascending: the
 * hit record that joins it to its representative as the join reports it (row < col), jorc and dist recomputed on the host with the C
 * library's log -- the reference's values bit for bit.  *n_links = genomes - representatives.
 * The hit records never leave the device (the frame of rk_forest_rows: the join through rk_dist_rows_dev with the threshold widened by
 * 2^-46 into max(65,536, rows * 64) records, once more with the exact count on overflow; the key pass with its small host buffer of
 * RK_CLUSTER_EDGE_CAP borderline records, run again alone on overflow).  Unlike a forest, the representatives cannot be patched
 * afterwards -- one kept borderline edge can flip representatives arbitrarily far away --, so the host decides the borderline records
 * BEFORE the rounds and sends the slot numbers of the kept ones back (8 bytes each, usually none).  Then decision rounds: an edge pass
 * marks the later endpoint of a record covered (the earlier one is a representative) or blocked for this round (both undecided), a
 * vertex pass turns undecided genomes into members (covered) or representatives (neither covered nor blocked); the host reads a counter
 * per round (per small batch of rounds later on) and stops when no genome is undecided.  Each round decides at least the first undecided
 * genome of the order: at most N rounds -- species cliques take 2-3, a path laid in priority order takes N.  Three sweeps then give every
 * member its nearest preceding representative (64-bit atomic minima on the weight key and on row << 32 | col).  PCIe traffic: 4 * N
 * bytes of order up, 44 * N bytes of representatives and links down, the borderline records and a counter per batch: never O(hits).
 * The rule does NOT compose from row shards the way components and forests do (whether a genome is a representative depends on every
 * genome before it): row_step > 1 is refused, and so is the join-only index of rk_index_join_shard, which holds one shard's rows.
 * RK_ERR_ARG: triangle != 1, null pointers, a row shard, a dense report (a threshold above 1.0), an index rk_dist_rows refuses for a
 * self join, a join-only index.  RK_ERR_UNSUPPORTED: a sketch of 2^30 hashes or more (the key), what the join answers, and a record
 * outside 0 < common <= u -- only sketches that repeat hashes produce such; the device key has no place for them (collections with
 * repeats whose records stay in range run normally).  An index without genomes: RK_OK, nothing runs, *links_out = NULL.  stats is
 * optional. */
typedef struct rk_greedy_stats {
    uint64_t edges;          /* hit records of the join */
    uint64_t borderline;     /* of which sent to the host */
    uint64_t borderline_kept;
    uint32_t join_attempts;  /* 2: the hit buffer overflowed once */
    uint32_t border_attempts; /* 2: the host buffer overflowed once */
    uint32_t rounds;         /* decision rounds up to the one that left no genome undecided; 0 when no record took part */
    uint32_t n_reps;         /* representatives, isolated genomes included */
} rk_greedy_stats;
int rk_greedy_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, const uint32_t *priority /* host, N, optional */,
                   uint32_t *rep_out /* host, N */, rk_hit **links_out, uint64_t *n_links, rk_greedy_stats *stats /* optional */);
/* Host only: the same rule over a hit list the caller already has (`metric` as rk_dist_opts.metric; one record per pair, as a join
 * reports them).  The links are the caller's records, unchanged.  With priority == NULL the sizes come from the records (triangle 1:
 * size0 = |S_row|, size1 = |S_col|); a genome without a record is isolated and needs none.  RK_ERR_ARG when records disagree about a
 * genome's size (priority == NULL), when a record names a genome >= n or has row == col, and for null pointers (hits may be NULL when
 * n_hits == 0). */
int rk_greedy_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, const uint32_t *priority /* n, optional */, int metric,
                   uint32_t *rep_out /* n */, rk_hit **links_out, uint64_t *n_links);

/* ---- k nearest neighbours --------------------------------------------------------- */
/* For every genome its k nearest neighbours within -D: the kNN graph of the all-vs-all -- the input of community detection, of
 * neighbour-graph layouts, of guide trees.  The graph is that of rk_cluster_rows: its edges are the pairs rk_dist_rows(ctx, idx, NULL,
 * opts, ...) would report -- same metric, same strict threshold decided with the C library's log, same row_first / row_step / row_block
 * selection, any index that call accepts, the join-only index of rk_index_join_shard included.
 * A record is INCIDENT to its row and to its col; the NEIGHBOUR of genome i in such a record is the other endpoint.  The list of genome
 * i holds the first min(k, degree(i)) incident records of the selected rows in this order: the ratio common / u descending, compared
 * exactly (u as in rk_forest_rows: 25/75 ties 20/60), then the neighbour's caller index ascending -- the order of rk_forest_rows
 * restricted to the records incident to one genome, whose (row, col) tie-break reads "neighbour ascending" there.  A record without a
 * ratio (u <= 0 or common < 0: only sketches that repeat hashes produce such) comes behind every record that has one.  The order is
 * strict, so the result is unique: it does not depend on the order of hits, the internal genome order, the join kernel or the sharding.
 * off_out[i] .. off_out[i + 1] (host, rk_index_genomes(idx) + 1 entries, i the caller index) delimit genome i's records in *nbrs_out
 * (library-allocated, rk_free_host; NULL when there is none), nearest first.  Each record is the hit record as the join reports it
 * (row < col), so a pair can appear in two lists; jorc and dist are recomputed on the host with the C library's log -- the reference's
 * values bit for bit.
 * Device path (stats.path == 1) for 1 <= k <= 64, one list slot per lane of a wave64.  The hit records never leave the device (the frame
 * of rk_forest_rows: the join through rk_dist_rows_dev with the threshold widened by 2^-46 into max(65,536, rows * 64) records, once more
 * with the exact count on overflow; the key pass with its small host buffer of RK_CLUSTER_EDGE_CAP borderline records, run again alone
 * on overflow).  A degree pass counts the live records per genome, two scans lay out a CSR adjacency of 16-byte entries {~ratio key,
 * neighbour << 32 | record number} and the output, a fill pass writes the entries, and a selection kernel -- one wave64 per genome, the
 * segment streamed in chunks of 64, a ballot filter against the current k-th, insertion by rank -- keeps the first k and writes their
 * hit records.  PCIe traffic: 4 * (N + 1) bytes of offsets, 40 bytes per returned record, the borderline records: never O(hits).  The
 * borderline records the host keeps are folded into their two endpoints' lists on the host (a kept edge changes only those two).
 * Inside the call, as rk_dist_rows + rk_knn_hits with the same result (stats.path == 2): k above 64, N * k >= 2^32, 2^31 hit records or
 * more, and RK_KNN_DEVICE=0.  k == 0: RK_OK, all offsets 0, nothing runs on the device (stats.path == 0); likewise an index without
 * genomes.
 * Row shards are accepted: a shard's call returns, for every genome, the first k of the records that shard owns; rk_knn_merge folds the
 * shards' results exactly -- the first k of a union are the first k of the union of the first ks.
 * RK_ERR_ARG: triangle != 1, null pointers, a dense report (a threshold above 1.0: pairs that share nothing carry no order), an index
 * rk_dist_rows refuses for a self join.  RK_ERR_UNSUPPORTED: a sketch of 2^30 hashes or more (the key), and what the join answers.
 * stats is optional. */
typedef struct rk_knn_stats {
    uint64_t edges;            /* hit records of the join */
    uint64_t borderline;       /* of which sent to the host */
    uint64_t borderline_kept;
    uint64_t neighbours;       /* records returned */
    uint32_t join_attempts;    /* 2: the hit buffer overflowed once */
    uint32_t border_attempts;  /* 2: the host buffer overflowed once */
    uint32_t max_degree;       /* most live records at one genome (device path) */
    uint32_t path;             /* 0 nothing ran, 1 device selection, 2 rk_dist_rows + rk_knn_hits inside the call */
} rk_knn_stats;                /* 48 bytes */
int rk_knn_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, uint32_t k, uint64_t *off_out /* host, N + 1 */,
                rk_hit **nbrs_out, uint64_t *n_nbrs, rk_knn_stats *stats /* optional */);
/* Host only: the same lists from a hit list the caller already has (`metric` as rk_dist_opts.metric; one record per pair, as a join
 * reports them); the records are returned unchanged.  RK_ERR_ARG when a record names a genome >= n or has row == col, and for null
 * pointers (hits may be NULL when n_hits == 0). */
int rk_knn_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, uint32_t k, int metric, uint64_t *off_out /* n + 1 */,
                rk_hit **nbrs_out, uint64_t *n_nbrs);
/* Host only: per genome, the first k of the union of two lists (a pair present in both counts once) -- what folds the results of row
 * shards and of GPUs into those of the collection.  Lists longer than k are cut to k; the lists need not be in order.  off_out may be
 * a_off or b_off.  RK_ERR_ARG: null pointers (a record array may be NULL when its lists are empty), offsets that do not ascend, a record
 * that names a genome >= n, has row == col or is not incident to the genome whose list holds it.  Nothing is written on a refusal. */
int rk_knn_merge(const uint64_t *a_off, const rk_hit *a, const uint64_t *b_off, const rk_hit *b, uint32_t n, uint32_t k, int metric,
                 uint64_t *off_out /* n + 1 */, rk_hit **out, uint64_t *n_out);

/* ---- density-based clusters ------------------------------------------------------- */
/* DBSCAN over the all-vs-all: clusters that do NOT chain.  Single linkage merges two species through one contaminated or chimeric
 * assembly that lies within -D of both; here such a genome joins them only if it is itself in a dense neighbourhood.
 * Graph.  The graph of rk_cluster_rows for ALL rows: its edges are the pairs rk_dist_rows(ctx, idx, NULL, opts, ...) would report --
 * same metric, same strict threshold (dist < max_dist decided with the C library's log).
 * Parameters and kinds.  deg(v) is the number of records incident to v.  min_pts >= 1 counts the genome itself, as scikit-learn's
 * min_samples does.  v is CORE iff deg(v) + 1 >= min_pts.
 * Clusters and labels.  Clusters are the connected components of the subgraph induced by the core genomes.  The label of a cluster is
 * the smallest caller index among its CORE genomes.  With min_pts = 1 the labels are those of rk_cluster_rows; with min_pts = 2 they
 * are those labels, with isolated genomes as noise.
 * Border genomes.  A non-core v with at least one core neighbour is BORDER.  It takes the label of its NEAREST core neighbour, in the
 * order of rk_forest_rows restricted to v: the ratio common / u descending, compared exactly (25/75 ties 20/60), then the core
 * neighbour's caller index ascending.  This is where textbook DBSCAN is order-dependent; here it is a function of the graph.  via[v]
 * names that neighbour.
 * Noise.  Every other non-core genome is noise: label = via = RK_DBSCAN_NOISE.
 * labels_out[v], kind_out[v] (0 noise, 1 border, 2 core), via_out[v] (RK_DBSCAN_NOISE unless v is border) and degree_out[v] = deg(v)
 * are host arrays of rk_index_genomes(idx) entries in the caller's genome order; via_out and degree_out are optional.  The result is
 * unique: it does not depend on the order of hits, the internal genome order or the kernel the join took.
 * The hit records never leave the device (the frame of rk_greedy_rows: the join through rk_dist_rows_dev with the threshold widened by
 * 2^-46 into max(65,536, rows * 64) records, once more with the exact count on overflow; the key pass with its small host buffer of
 * RK_CLUSTER_EDGE_CAP borderline records and their slot numbers, run again alone on overflow).  One kept borderline edge can make a
 * genome core and merge two clusters arbitrarily far away, so the host decides the borderline records BEFORE any degree is counted and
 * sends the slot numbers of the kept ones back (8 bytes each, usually none).  Then three sweeps over the keyed records -- the degrees; the
 * hook (both endpoints core: the compare-and-swap link of rk_cluster_rows; exactly one core: a 64-bit atomic minimum of the weight key
 * at the other); the border settle (a 32-bit atomic minimum of the core neighbour's index among the records that match that key) --
 * and one pass per genome that writes kind, label, via and degree.  PCIe traffic: 13 * N bytes of results, four counters and the
 * borderline records: never O(hits).
 * The core test does NOT compose from row shards (the degrees of a shard are partial): row_step > 1 is refused, and so is the join-only
 * index of rk_index_join_shard, which holds one shard's rows.  RK_DBSCAN_DEVICE=0 answers inside the call as rk_dist_rows +
 * rk_dbscan_hits, with the same result.
 * RK_ERR_ARG: triangle != 1, null pointers (labels_out, kind_out), min_pts == 0, a row shard, a dense report (a threshold above 1.0),
 * an index rk_dist_rows refuses for a self join, a join-only index.  RK_ERR_UNSUPPORTED: a sketch of 2^30 hashes or more (the key),
 * what the join answers, and a record outside 0 < common <= u -- only sketches that repeat hashes produce such; it has no place in the
 * nearness order (collections with repeats whose records stay in range run normally).  An index without genomes: RK_OK, nothing
 * runs.  stats is optional. */
#define RK_DBSCAN_NOISE 0xFFFFFFFFu
typedef struct rk_dbscan_stats {
    uint64_t edges;          /* hit records of the join */
    uint64_t borderline;     /* of which sent to the host */
    uint64_t borderline_kept;
    uint32_t join_attempts;  /* 2: the hit buffer overflowed once */
    uint32_t border_attempts; /* 2: the host buffer overflowed once */
    uint32_t n_clusters;     /* components of the core genomes */
    uint32_t n_core;
    uint32_t n_border;
    uint32_t n_noise;
} rk_dbscan_stats;           /* 48 bytes */
int rk_dbscan_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, uint32_t min_pts, uint32_t *labels_out /* host, N */,
                   uint8_t *kind_out /* host, N: 0 noise, 1 border, 2 core */, uint32_t *via_out /* host, N, optional */,
                   uint32_t *degree_out /* host, N, optional */, rk_dbscan_stats *stats /* optional */);
/* Host only: the same rule over a hit list the caller already has (`metric` as rk_dist_opts.metric; one record per pair, as a join
 * reports them).  RK_ERR_ARG when a record names a genome >= n or has row == col, for min_pts == 0 and for null pointers (hits may be
 * NULL when n_hits == 0; via_out and degree_out are optional).  Nothing is written on a refusal. */
int rk_dbscan_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, uint32_t min_pts, int metric, uint32_t *labels_out /* n */,
                   uint8_t *kind_out /* n */, uint32_t *via_out /* n, optional */, uint32_t *degree_out /* n, optional */);

/* ---- mutual-reachability forest ---------------------------------------------------- */
/* The minimum spanning forest of the all-vs-all under MUTUAL-REACHABILITY distance: the HDBSCAN* hierarchy up to -D, the density
 * counterpart of rk_forest_rows.  Cut at any t <= D it gives the core genomes and the clusters rk_dbscan_rows returns at t, without a
 * join; with min_pts = 1 it is rk_forest_rows' forest.
 * Graph.  That of rk_cluster_rows for ALL rows: the pairs `alldist -D d` reports -- rk_dist_rows(ctx, idx, NULL, opts, ...) --, with the
 * strict `<` on the C library's distance.
 * Core record.  min_pts >= 1 counts the genome itself, as in rk_dbscan_rows.  Let k = min_pts - 1.  For k >= 1 the core record of v is
 * the k-th entry of v's neighbour list in the order of rk_knn_rows: ratio descending, compared exactly, then the neighbour's caller
 * index ascending.  core_dist[v] is that record's dist, recomputed on the host with the C library's log; core_nb[v] is the neighbour.  A
 * genome with fewer than k incident records has no core record: core_dist[v] = +inf and core_nb[v] = RK_MREACH_NONE; such a genome is
 * noise at every level <= D and no edge touches it.  For k = 0, core_dist[v] = 0.0 and core_nb[v] = RK_MREACH_NONE for every v.
 * Weight.  The weight of record e = (a, b) is mw(e) = max(w(e), core_w[a], core_w[b]), where w is the nearness weight of
 * rk_forest_rows' order (it rises as the ratio common / u falls) and core_w[v] is the w of v's core record, 0 for k = 0 and infinite
 * for a genome without one.  In doubles this is max(e.dist, core_dist[row], core_dist[col]).
 * Order of edges.  mw ascending and exact (25/75 ties 20/60), then row ascending, then col ascending (row < col, as a join reports a
 * pair).  The order is strict, so the forest is unique: the edges Kruskal accepts in this order among the records with finite mw.
 * *edges_out (library-allocated, rk_free_host) lists them in this order: rk_hit records of the underlying pairs,
 * at most N - 1 of them, jorc and dist bit for bit the reference's.  The result does not depend on the order of hits or genomes, nor on
 * the kernel the join took.  core_dist_out (host, N doubles) is required, core_nb_out (host, N) and stats are optional.
 * The hit records never leave the device (the frame of rk_dbscan_rows: the join through rk_dist_rows_dev with the threshold widened by
 * 2^-46, the key pass with its small host buffer of RK_CLUSTER_EDGE_CAP borderline records and their slot numbers, both retries).  One
 * kept borderline edge changes a core distance and with it the weight of edges arbitrarily far away, so the host decides the borderline
 * records BEFORE anything else and sends the slot numbers of the kept ones back.  Then, for k >= 1, the degrees, a scan, the CSR
 * adjacency of rk_knn_rows and its wave64 selection, which here keeps the k-th entry alone; one sweep that raises every record's weight
 * to mw; the Boruvka rounds of rk_forest_rows over mw (at most 2 + ceil(log2 N)); a sort of the forest by (mw, row, col).  PCIe
 * traffic: 40 bytes per edge and 40 bytes per genome (its core record), the borderline records and a counter per round: never O(hits).
 * Inside the call, as rk_dist_rows + rk_mreach_hits with the same result (stats.path == 2): min_pts above 65 (k above 64, the lanes of
 * a wave64), 2^31 hit records or more, and RK_MREACH_DEVICE=0.
 * The core distances do NOT compose from row shards: row_step > 1 is refused, and so is the join-only index of rk_index_join_shard.
 * RK_ERR_ARG: triangle != 1, null pointers (core_dist_out, edges_out, n_edges), min_pts == 0, a row shard, a dense report (a threshold
 * above 1.0), an index rk_dist_rows refuses for a self join, a join-only index.  RK_ERR_UNSUPPORTED: a sketch of 2^30 hashes or more
 * (the key), what the join answers, and a record outside 0 < common <= u (only sketches that repeat hashes produce such).  An index
 * without genomes: RK_OK, nothing runs, *edges_out = NULL. */
#define RK_MREACH_NONE 0xFFFFFFFFu
typedef struct rk_mreach_stats {
    uint64_t edges;          /* hit records of the join */
    uint64_t borderline;     /* of which sent to the host */
    uint64_t borderline_kept;
    uint32_t join_attempts;  /* 2: the hit buffer overflowed once */
    uint32_t border_attempts; /* 2: the host buffer overflowed once */
    uint32_t rounds;         /* Boruvka rounds, the last (empty) one included; 0 when no record took part */
    uint32_t n_trees;        /* genomes minus returned edges: components, singletons and genomes without a core record included */
    uint32_t n_core;         /* genomes with a finite core distance */
    uint32_t max_degree;     /* most live records at one genome (device path, min_pts >= 2) */
    uint32_t path;           /* 0 nothing ran, 1 device, 2 rk_dist_rows + rk_mreach_hits inside the call */
    uint32_t pad_;
} rk_mreach_stats;           /* 56 bytes */
int rk_mreach_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, uint32_t min_pts, double *core_dist_out /* host, N */,
                   uint32_t *core_nb_out /* host, N, optional */, rk_hit **edges_out, uint64_t *n_edges,
                   rk_mreach_stats *stats /* optional */);
/* Host only: the same rule over a hit list the caller already has (`metric` as rk_dist_opts.metric; one record per pair, as a join
 * reports them).  The edges are the caller's records, unchanged; core_dist is the core record's dist field as the caller gave it.  A
 * record with row > col counts as the pair (col, row) in the order.  A record without a ratio (u <= 0 or common < 0) weighs more than
 * every record that has one.  RK_ERR_ARG when a record names a genome >= n or has row == col, for min_pts == 0 and for null pointers
 * (hits may be NULL when n_hits == 0, core_dist_out when n == 0; core_nb_out is optional). */
int rk_mreach_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, uint32_t min_pts, int metric, double *core_dist_out /* n */,
                   uint32_t *core_nb_out /* n, optional */, rk_hit **edges_out, uint64_t *n_edges);
/* Host only: the forest cut at t <= D, in the form of rk_dbscan_rows' labels.  Genome v is core at t iff core_dist[v] < t; an edge links
 * iff max(dist, core_dist[row], core_dist[col]) < t; labels_out[v] = the smallest index of v's component among the core genomes, or
 * RK_DBSCAN_NOISE for a genome that is not core at t.  This is DBSCAN*: a BORDER genome of rk_dbscan_rows at t is noise here, because
 * the forest does not hold the edges that would assign it.  The core genomes and their labels are those of rk_dbscan_rows at t with the
 * same min_pts.  (At t = 0 no genome is core, whatever min_pts: no distance lies below 0.)  RK_ERR_ARG for an edge that names a genome >= n or null pointers (edges may be NULL when n_edges == 0). */
int rk_mreach_cut(const rk_hit *edges, uint64_t n_edges, const double *core_dist /* n */, uint32_t n, double t, uint32_t *labels_out /* n */);

/* ---- medoids and census of a clustering --------------------------------------------- */
/* What a user does next with the labels of rk_cluster_rows, rk_dbscan_rows, rk_forest_cut, rk_mreach_cut or rep_out of rk_greedy_rows:
 * pick a representative by centrality (the member with the highest summed similarity to its fellow members, as dRep, GTDB and galah
 * print it) and check the clustering (how dense a cluster is, its weakest pair, every genome's nearest genome outside its cluster).
 * All of it is sums and extrema over the hit records, grouped by a label array of N words.
 * Graph.  The graph of rk_cluster_rows: its edges are the pairs rk_dist_rows(ctx, idx, NULL, opts, ...) would report -- same metric, same
 * strict threshold (dist < max_dist decided with the C library's log), same row_first / row_step / row_block selection, any index that
 * call accepts, the join-only index of rk_index_join_shard included.
 * Labels.  labels[v] (host, rk_index_genomes(idx) = N entries in the caller's genome order): a value below N names v's cluster -- it
 * need not be a member of that cluster --, RK_MEDOID_NONE (the value of RK_DBSCAN_NOISE) means v is unlabelled; anything else is
 * RK_ERR_ARG.  The outputs of the five calls above are all of this form.
 * Inside and leaving.  A record (a, b) is INSIDE iff labels[a] == labels[b] != RK_MEDOID_NONE; otherwise it is LEAVING, for both of its
 * ends.  An unlabelled genome has only leaving records.
 * Similarity term.  q(e) = floor(common * 2^32 / u), u as in rk_forest_rows (size0 + size1 - common for metric 0, min(size0, size1) for
 * metric 1): the jaccard or containment of the record in 32 fractional bits, exact for 0 < common <= u < 2^31.  q <= 2^32, a genome has
 * fewer than N records and N <= 2^31 is required (RK_ERR_UNSUPPORTED beyond): a genome's sum stays below 2^63.
 * Per genome v.  in_deg[v] and out_deg[v]: the inside and the leaving records incident to v.  central[v]: the sum of q over v's inside
 * records -- a pair beyond -D is not reported and contributes 0.  far_in[v]: the inside record incident to v with the SMALLEST ratio
 * common / u, compared exactly (25/75 ties 20/60); ties go to the smaller neighbour index.  near_out[v]: the leaving record incident to v
 * with the LARGEST ratio; ties go to the smaller neighbour index -- the first leaving record of v in the order of rk_knn_rows.  The two
 * record arrays are optional.  Each entry is the hit record as the join reports it (row < col, pad_ 0), jorc and dist recomputed on the
 * host with the C library's log -- the reference's values bit for bit; an absent record has row = col = RK_MEDOID_NONE and zeros
 * elsewhere.  The result is unique: it does not depend on the order of hits, the internal genome order, the join kernel or the sharding.
 * "Medoid" here MAXIMISES SUMMED SIMILARITY over the reported pairs; it does not minimise summed distance.  An unreported pair has a
 * bound on its similarity from above that is safe to sum (0 for a pair that shares nothing, below the ratio at -D otherwise: counted as
 * 0) and no distance at all: a sum of distances over the reported pairs alone would favour the member with the FEWEST neighbours.
 * Per non-empty cluster l (rk_medoid_pick, host work over the per-genome arrays).  size; in_edges: the sum of in_deg over the members,
 * halved; medoid: the member with the largest central, ties to the smaller caller index (a singleton is its own medoid) and central:
 * the medoid's; weakest_in: over the members' far_in the record with the smallest ratio, ties to the smaller (row, col); nearest_out:
 * over the members' near_out the record with the largest ratio, ties to the smaller (row, col) -- both absent without the two record
 * arrays.  Clusters come by ascending label in *out (library-allocated, rk_free_host; NULL when there is none).
 * The hit records never leave the device (the frame of rk_dbscan_rows: the join through rk_dist_rows_dev with the threshold widened by
 * 2^-46, the key pass with its small host buffer of RK_CLUSTER_EDGE_CAP borderline records and their slot numbers, both retries; the host
 * decides the borderline records BEFORE anything is summed and sends the slot numbers of the kept ones back).  The labels go up once
 * (4 * N bytes).  Then a sums sweep (per live record two label loads, integer atomic adds on both ends' degree and, inside, on central; a
 * 64-bit atomic maximum of the weight key at both ends of an inside record, a 64-bit atomic minimum at both ends of a leaving one), a
 * settle sweep (a 32-bit atomic minimum of the neighbour's index among the records that match a genome's extreme key) and a gather of
 * the winning records; the last two are skipped when no record array is asked for.  One read-back of 16 * N bytes, 96 * N with the
 * records, and the borderline records: never O(hits).
 * Row shards and GPUs compose exactly (sums add, extrema of a union are extrema of the extrema): rk_medoid_merge folds the results of
 * two DISJOINT record sets -- degrees and central add, far_in keeps the farther record and near_out the nearer in the orders above, an
 * absent record loses; a record array is written only where both inputs and out have it; out may alias a.
 * RK_MEDOID_DEVICE=0 answers inside the call as rk_dist_rows + rk_medoid_hits, with the same result.
 * RK_ERR_ARG: triangle != 1, null pointers (labels, out, out->in_deg, out->out_deg, out->central), a label that is neither below N nor
 * RK_MEDOID_NONE, a dense report (a threshold above 1.0), an index rk_dist_rows refuses for a self join.  RK_ERR_UNSUPPORTED: a sketch of
 * 2^30 hashes or more (the key), what the join answers, and a record outside 0 < common <= u -- only sketches that repeat hashes
 * produce such; q is not defined for them.  Nothing is written on a refusal.  An index without genomes: RK_OK, nothing runs.  stats is
 * optional. */
#define RK_MEDOID_NONE 0xFFFFFFFFu
typedef struct rk_medoid_genomes {   /* the caller's arrays of n entries; far_in / near_out may be NULL */
    uint32_t *in_deg, *out_deg;
    uint64_t *central;
    rk_hit *far_in, *near_out;
} rk_medoid_genomes;
typedef struct rk_medoid_cluster {
    uint32_t label, size, medoid, pad_;
    uint64_t in_edges, central;      /* inside records of the cluster; central[medoid] */
    rk_hit weakest_in, nearest_out;
} rk_medoid_cluster;                 /* 112 bytes */
typedef struct rk_medoid_stats {
    uint64_t edges;          /* hit records of the join */
    uint64_t borderline;     /* of which sent to the host */
    uint64_t borderline_kept;
    uint64_t inside;         /* records of the graph with both ends in one cluster */
    uint64_t leaving;        /* the others */
    uint32_t join_attempts;  /* 2: the hit buffer overflowed once */
    uint32_t border_attempts; /* 2: the host buffer overflowed once */
} rk_medoid_stats;           /* 48 bytes */
int rk_medoid_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, const uint32_t *labels /* host, N */, rk_medoid_genomes *out,
                   rk_medoid_stats *stats /* optional */);
/* Host only: the same rule over a hit list the caller already has (`metric` as rk_dist_opts.metric; one record per pair, as a join
 * reports them).  The two records of a genome are the caller's, unchanged but for their orientation: a record with row > col is returned
 * as the pair (col, row), its sizes swapped with it.  RK_ERR_ARG when a record names a genome >= n or has row == col, for a label that is
 * neither below n nor RK_MEDOID_NONE and for null pointers (hits may be NULL when n_hits == 0, everything but out when n == 0);
 * RK_ERR_UNSUPPORTED for a record outside 0 < common <= u and for n above 2^31.  Nothing is written on a refusal. */
int rk_medoid_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, const uint32_t *labels /* n */, int metric, rk_medoid_genomes *out);
/* Host only: folds the results of two disjoint record sets (row shards, GPUs) as described above.  RK_ERR_ARG for null pointers and for
 * a present record that names a genome >= n, has row >= col or is not incident to the genome whose entry holds it.  Nothing is written
 * on a refusal. */
int rk_medoid_merge(const rk_medoid_genomes *a, const rk_medoid_genomes *b, uint32_t n, int metric, rk_medoid_genomes *out);
/* Host only: the per-cluster records from the per-genome arrays, by ascending label.  g->far_in and g->near_out are needed for
 * weakest_in and nearest_out alone: without BOTH arrays those two are absent.  RK_ERR_ARG for null pointers (labels and the arrays of g
 * may be NULL when n == 0) and for a label that is neither below n nor RK_MEDOID_NONE. */
int rk_medoid_pick(const uint32_t *labels /* n */, const rk_medoid_genomes *g, uint32_t n, int metric, rk_medoid_cluster **out,
                   uint32_t *n_out);

/* ---- placement of query genomes into a labelled collection --------------------------- */
/* What a user does next with a clustered collection and NEW genomes: for each query, which cluster it belongs to, how well supported
 * that placement is, which cluster is the runner-up, whether the genome is novel.  All of it is sums and extrema over the hit records
 * of the QUERY join, grouped by a label array of N words.
 * Graph.  The records rk_dist_rows(ctx, idx, queries, opts, ...) would report with triangle = 0 -- same metric, the reference's NON-strict
 * threshold (dist <= max_dist decided with the C library's log), same row_first / row_step / row_block selection of QUERY rows.  A
 * record has row = query, col = reference, size0 = |reference|, size1 = |query|.
 * Labels.  labels[r] (host, rk_index_genomes(idx) = N entries in the caller's reference order): a value below N names r's cluster,
 * RK_ASSIGN_NONE (the value of RK_DBSCAN_NOISE) means r is unlabelled; anything else is RK_ERR_ARG.  The outputs of rk_cluster_rows,
 * rk_dbscan_rows, rk_forest_cut, rk_mreach_cut and rep_out of rk_greedy_rows are all of this form; for DBSCAN "predict" the caller sets
 * the non-core genomes to RK_ASSIGN_NONE.  An unlabelled reference is counted but never anchors a query.
 * Per selected query q.  n_within[q]: q's records.  n_labelled[q]: those whose reference is labelled.  nearest[q]: the record of q's
 * nearest LABELLED reference in the order of rk_knn_rows restricted to q: the ratio common / u descending, compared exactly (25/75 ties
 * 20/60), then the reference's caller index ascending; u as in rk_forest_rows (size0 + size1 - common for metric 0, min(size0, size1)
 * for metric 1).  label[q] = labels[nearest[q].col], or RK_ASSIGN_NONE when q has no labelled record: such a q is NOVEL.  n_same[q]: q's
 * records whose reference carries label[q] -- the support of the placement (0 for a novel q).  runner_up[q]: the nearest record of q,
 * in the same order, whose reference is labelled with a label OTHER than label[q] -- how ambiguous the placement is; absent when
 * there is none.  An absent record (nearest of a novel q, a missing runner-up) has row = col = RK_ASSIGN_NONE and zeros elsewhere, as
 * rk_medoid_rows writes them.
 * Records.  The two record arrays are optional.  A present record is the hit as the join reports it (pad_ 0), jorc and dist recomputed
 * on the host with the C library's log -- the reference's values bit for bit.
 * The result is unique: it does not depend on the order of hits, the internal genome order or the query kernel the join took.
 * Entries of unselected query rows are NOT WRITTEN, and a query's result depends on its own records alone: row shards and GPUs
 * compose by writing into one set of arrays, no merge call is needed.  (Sharding by REFERENCES is not offered: n_same does not compose.)
 * The hit records never leave the device (the frame of rk_medoid_rows over the query join: rk_dist_rows_dev with the threshold widened
 * by 2^-46, the key pass with its small host buffer of RK_CLUSTER_EDGE_CAP borderline records and their slot numbers, both retries; the
 * host decides the borderline records with `<=` BEFORE anything is counted and sends the slot numbers of the kept ones back).  The
 * labels go up once (4 * N bytes).  Then: a first sweep (integer atomic adds on n_within and n_labelled, a 64-bit atomic minimum of
 * the weight key of a labelled record at its query), a settle sweep (a 32-bit atomic minimum of the reference's index among the records
 * that match their query's key), one thread per query for label[q], a second sweep (the add on n_same, the 64-bit minimum among the
 * other labels), its settle sweep and a gather of the winning records; the 64-bit minimum of the second sweep, its settle sweep and the
 * gather are skipped when no record array is asked for.  One read-back of 16 * Q bytes, 96 * Q with the records, and the borderline
 * records: never O(hits).
 * RK_ASSIGN_DEVICE=0 answers inside the call as rk_dist_rows + rk_assign_hits, with the same result; so does a join of 2^31 records or more.
 * RK_ERR_ARG: triangle != 0, queries == NULL, null pointers (labels, out, out->label, out->n_within, out->n_labelled, out->n_same), a
 * label that is neither below N nor RK_ASSIGN_NONE, a dense report (triangle = 0: a threshold of 1.0 or above), an index without posting
 * lists (the join-only index of rk_index_join_shard, a shard of a sharded build), what rk_dist_rows refuses for explicit queries.
 * RK_ERR_UNSUPPORTED: a reference or query sketch of 2^30 hashes or more (the key), what the join answers, and a record outside
 * 0 < common <= u -- only sketches that repeat hashes produce such; they have no place in the order.  Nothing is written on a refusal.
 * No queries: RK_OK, nothing runs.  An index without genomes: RK_OK, no join runs, every selected query is novel.  stats is optional. */
#define RK_ASSIGN_NONE 0xFFFFFFFFu
typedef struct rk_assign_queries {   /* the caller's arrays of Q = rk_sketches_count(queries) entries; nearest / runner_up may be NULL */
    uint32_t *label, *n_within, *n_labelled, *n_same;
    rk_hit *nearest, *runner_up;
} rk_assign_queries;
typedef struct rk_assign_stats {
    uint64_t edges;          /* hit records of the join */
    uint64_t borderline;     /* of which sent to the host */
    uint64_t borderline_kept;
    uint32_t join_attempts;  /* 2: the hit buffer overflowed once */
    uint32_t border_attempts; /* 2: the host buffer overflowed once */
    uint32_t placed;         /* selected queries with a label */
    uint32_t novel;          /* selected queries without */
    uint32_t ambiguous;      /* placed queries with a runner-up (n_labelled > n_same) */
    uint32_t sweeps;         /* sweeps over the records behind the stage: 5 with a record array, 3 without, 0 on the host path */
} rk_assign_stats;           /* 48 bytes */
int rk_assign_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_dist_opts *opts, const uint32_t *labels /* host, N */,
                   rk_assign_queries *out, rk_assign_stats *stats /* optional */);
/* Host only: the same rule over a hit list the caller already has (row = query below n_query, col = reference below n_ref; `metric` as
 * rk_dist_opts.metric; one record per pair, as a join reports them).  EVERY entry of the n_query rows is written; the records are the
 * caller's, unchanged.  RK_ERR_ARG when a record names a query >= n_query or a reference >= n_ref, for a label that is neither below
 * n_ref nor RK_ASSIGN_NONE and for null pointers (hits may be NULL when n_hits == 0, labels when n_ref == 0, the arrays of out when
 * n_query == 0); RK_ERR_UNSUPPORTED for a record outside 0 < common <= u.  Nothing is written on a refusal. */
int rk_assign_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n_query, uint32_t n_ref, const uint32_t *labels /* n_ref */, int metric,
                   rk_assign_queries *out);

/* ---- pan, core and marker sketches per cluster --------------------------------------- */
/* What turns a labelled collection back into sketches: per cluster the union of its members' sketches (its pan sketch), the hashes
 * every member holds (its core sketch), the hashes no genome outside it holds (its markers) -- the reference's `union` and `sub`
 * (src/subCommand.cpp:307-543, :545-794) for every cluster at once, from the posting lists alone: no join, no distance.
 * Labels.  labels[v] (host, rk_index_genomes(idx) = N entries in the caller's genome order): a value below N names v's cluster (it need
 * not be a member of it), RK_GROUP_NONE (the value of RK_DBSCAN_NOISE) means v is unlabelled; anything else is RK_ERR_ARG.  The GROUPS
 * are the labels in use by ascending label, K of them; m_l = the genomes that carry l (one with an empty sketch counts).
 * Rule (integers only).  For a hash h: c_l(h) = the DISTINCT genomes labelled l whose sketch holds h (a sketch that repeats h counts
 * once), t(h) = the distinct genomes that hold h, unlabelled ones included.  h is in the sketch of group l iff c_l(h) >= min_count and
 * c_l(h) * share_den >= share_num * m_l (64-bit products) and, with only = 1, c_l(h) == t(h): every holder carries l -- an unlabelled
 * holder is outside every cluster and defeats it.  pan {0,1,1,0}, core {1,1,1,0}, majority {1,2,1,0}, markers {0,1,1,1}.
 * Result.  *out: K sketches by ascending label, each strictly ascending, of the hash width of the index, device-resident and
 * library-owned (rk_sketches_free): it goes straight into rk_index_build, rk_dist_rows, rk_dist_topn, rk_assign_rows.  A group without a
 * hash is an empty sketch.  group_label_out / group_size_out: K entries each, the label and m_l (rk_free_host).  The result is unique:
 * it does not depend on the internal genome order, on how the index came to be or on the path taken.
 * Accepted: every index that carries posting lists, built (rk_index_build) or imported (rk_index_import, rk_index_import64).
 * The host computes need[g] = max(min_count, ceil(share_num * m / share_den)); 4 * N + 4 * K bytes go up, the counters and 8 * (K + 1)
 * bytes of offsets come back, never the postings.  On the device (rk_group.hip): the group numbers in internal order, then per posting
 * list by its length -- up to lane_max postings one lane, up to wave_max one wave, beyond that a workgroup that streams the list in
 * chunks of `chunk` postings into an LDS table of table_groups groups; a list with more groups than the table holds is SPILLED: its
 * raw keys are sorted and run-length counted.  A (group, list) that passes appends one 64-bit key; the keys are sorted, the offsets of
 * the groups found, the hashes gathered.  When the key buffer (or the spill buffer) overflows, the call runs once more with the exact
 * count (attempts = 2); RK_GROUP_CAP / RK_GROUP_SPILL_CAP (developer switches) set the first capacities.
 * RK_GROUP_DEVICE=0 answers inside the call as export + rk_group_lists + rk_sketches_from_host(64), with the same result.
 * RK_ERR_ARG: null pointers, a label that names nothing, share_den == 0, share_num > share_den, min_count == 0, only > 1, an index
 * without posting lists (the join-only index of rk_index_join_shard), one hash range of a sharded build.  RK_ERR_UNSUPPORTED: more than
 * 2^31 genomes.  Nothing is written on a refusal.  No genomes, or no labelled genome: RK_OK, nothing runs, *out = NULL, *n_groups = 0,
 * the two arrays NULL.  stats is optional. */
#define RK_GROUP_NONE 0xFFFFFFFFu
#define RK_MS_GROUP 13          /* rk_group_sketches: the first list kernel through the gather of the hashes; 0 on the host path */
typedef struct rk_group_rule {
    uint32_t share_num, share_den;  /* 0 <= num <= den, den >= 1 */
    uint32_t min_count;             /* >= 1 */
    uint32_t only;                  /* 0 or 1 */
} rk_group_rule;
typedef struct rk_group_stats {
    uint64_t lists;          /* posting lists = distinct hashes of the index */
    uint64_t postings;
    uint64_t kept;           /* (group, hash) pairs of the result = rk_sketches_total(*out) */
    uint64_t lane_lists;     /* lists of up to lane_max postings: one lane each */
    uint64_t wave_lists;     /* lists of up to wave_max postings: one wave each */
    uint64_t block_lists;    /* longer lists: one workgroup each, streamed in chunks (the spilled ones included) */
    uint64_t spilled;        /* of which with more than table_groups groups: counted by sort + run lengths */
    uint32_t labelled;       /* genomes with a label */
    uint32_t groups;         /* K */
    uint32_t attempts;       /* 2: the key buffer or the spill buffer overflowed once; 0 when nothing ran or on the host path */
    uint32_t path;           /* 0 nothing ran, 1 device, 2 host */
    uint32_t lane_max, wave_max, table_groups, chunk;   /* the constants of the list kernels (every path fills them) */
} rk_group_stats;            /* 88 bytes */
int rk_group_sketches(rk_ctx *ctx, const rk_index *idx, const uint32_t *labels /* host, N */, const rk_group_rule *rule, rk_sketches **out,
                      uint32_t **group_label_out, uint32_t **group_size_out, uint32_t *n_groups, rk_group_stats *stats /* optional */);
/* Host only: the same rule over posting lists as rk_index_export_lists / rk_index_export64 return them (the lists back to back in
 * `postings`, their lengths in `counts`; genome ids below n_genomes in any order within a list, repeats allowed and counted once).  Per
 * group the INDICES of the kept lists, ascending: kept_out[off_out[g] .. off_out[g + 1]) -- blind to the hash width, the caller maps an
 * index to its hash.  off_out has K + 1 entries; kept_out, group_label_out and group_size_out are NULL when they would be empty; all
 * four are the library's (rk_free_host).  RK_ERR_ARG for a posting >= n_genomes, a bad label or rule, null pointers (postings / counts
 * may be NULL when n_lists is 0 or every list is empty, labels when n_genomes is 0).  Nothing is written on a refusal. */
int rk_group_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, uint32_t n_genomes, const uint32_t *labels /* n_genomes */,
                   const rk_group_rule *rule, uint64_t **off_out /* K + 1 */, uint64_t **kept_out, uint32_t **group_label_out, uint32_t **group_size_out,
                   uint32_t *n_groups);

/* ---- decomposing queries into references --------------------------------------------- */
/* rk_gather_rows: which references explain a query sketch, in what order, and how much each adds beyond the ones already chosen -- the
 * greedy minimum set cover (sourmash `gather`) of every selected query over the references of an index, in integers only.  Sketches are
 * taken as SETS: an index whose references repeat a hash and queries that repeat a hash are RK_ERR_UNSUPPORTED.
 * Per selected query q with hash set S: matched[q] = the hashes of S that have a posting list; common(r) = |S n R_r|; n_cand[q] = the
 * references with common(r) >= min_new.  Rounds: M_0 = the matched hashes of S; in round t, rem_t(r) = |M_t n R_r| over the references
 * not yet picked; the pick is the reference with the largest rem_t, ties to the smaller CALLER's reference index; the rounds end when
 * that maximum is below min_new or when t = max_picks (0: no limit); otherwise M_{t+1} = M_t \ R_pick.  One record per pick:
 * rank = t, common = the original overlap, fresh = rem_t(pick), left = |M_{t+1}|, the two sketch sizes.  covered[q] = the sum of fresh.
 * off_out (host, Q + 1 entries, every one written; an unselected row is empty) delimits the picks of each query in *picks_out
 * (library-allocated, rk_free_host; NULL when there is none), which come in (query, rank) order.  matched_out / n_cand_out / covered_out
 * (host, Q entries each): only the entries of the selected rows (row_first / row_step / row_block as in rk_dist_opts) are written.
 * The result is unique: it does not depend on the internal genome order, on how the index came to be (built or imported), on batches,
 * on shards or on the path taken.  With min_new = 1 and max_picks = 0, covered == matched for every query.  A query's result depends on
 * its own hashes alone: row shards compose by concatenation, no merge call is needed.
 * On the device (rk_gather.hip), per batch of query rows whose counter rows fit RK_GATHER_BATCH_BYTES (default 1 GiB; at least one row):
 * the counter rows of the query join (stage A of rk_dist_topn) become the mutable rem; the candidates (ref, common) with common >= min_new
 * and the matched posting lists are compacted per batch; then two kernels per round over the whole batch: one workgroup per live row
 * takes the maximum of (rem, -ref) over the row's candidates and appends the pick, then every live matched list of a live row looks for
 * the winner by binary search (a list ascends in internal genome id) and, on a hit, dies and takes 1 off rem of every genome it names
 * (relaxed agent-scope integer adds) -- by one lane up to lane_max postings, by one wave up to wave_max, by the workgroup beyond.  The
 * host reads the number of live rows every sync_every rounds and launches nothing once it is 0; the live lists are compacted when
 * fewer than half survive.  One read-back carries 32 picks + 12 Q + 8 (Q + 1) bytes; counter rows and postings never leave the device.
 * RK_GATHER_DEVICE=0 answers inside the call as export + rk_gather_lists, with the same result; stats->path says which leg ran.
 * RK_ERR_ARG: null pointers, min_new == 0, an index without posting lists (the join-only index of rk_index_join_shard, one hash range of
 * a sharded build), queries and index of different hash widths.  RK_ERR_UNSUPPORTED: sketches that repeat a hash, and an index of
 * 2^31 - 1 postings or more (as rk_dist_rows answers explicit queries).  Nothing is written on a refusal.  No query: RK_OK, nothing runs.
 * An index without genomes: RK_OK, every row empty. */
#define RK_MS_GATHER 14         /* rk_gather_rows: the counts of the first batch through the last compaction of picks; 0 on the host path */
typedef struct rk_gather_opts {
    uint32_t min_new;        /* >= 1: a pick adds at least this many hashes that no earlier pick held */
    uint32_t max_picks;      /* picks per query at most; 0: no limit */
    uint32_t row_first, row_step, row_block;   /* the row shard, as in rk_dist_opts (0 0 0: every query) */
} rk_gather_opts;            /* 20 bytes */
typedef struct rk_gather_pick {
    uint32_t query, ref;     /* the query row and the CALLER's reference index */
    uint32_t rank;           /* t: the round of the pick, from 0 */
    uint32_t common;         /* |S n R_ref|, the original overlap */
    uint32_t fresh;          /* rem_t(ref): matched hashes of the query that no earlier pick held */
    uint32_t left;           /* |M_{t+1}|: matched hashes still unexplained after this pick */
    uint32_t size_ref, size_query;
} rk_gather_pick;            /* 32 bytes */
typedef struct rk_gather_stats {
    uint64_t picks, candidates, matched;   /* sums over the selected rows */
    uint64_t decrements;     /* postings of the lists that died on a winner (device leg); the lists of a row's LAST pick are not walked when nothing is left */
    uint64_t lane_lists, wave_lists, block_lists;   /* lists that died, by who walked them (device leg) */
    uint64_t rows_per_batch;
    uint32_t path;           /* 0 nothing ran, 1 the device, 2 the host (RK_GATHER_DEVICE=0) */
    uint32_t rows;           /* selected rows */
    uint32_t batches;
    uint32_t rounds;         /* the most picks of any row: the rounds that did work */
    uint32_t launched_rounds;   /* rounds the host launched, all batches; at most sync_every - 1 more per batch than the batch needed, plus the one that retires */
    uint32_t launches;       /* kernels of this unit the host launched */
    uint32_t read_backs;     /* synchronising reads of the counters */
    uint32_t compactions;    /* of the live lists */
    uint32_t lane_max, wave_max, sync_every, threads;   /* the constants of the round kernels (every path fills them) */
} rk_gather_stats;           /* 112 bytes */
int rk_gather_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_gather_opts *opts, uint64_t *off_out /* host, Q + 1 */,
                   rk_gather_pick **picks_out, uint64_t *n_picks, uint32_t *matched_out /* host, Q */, uint32_t *n_cand_out /* host, Q */,
                   uint32_t *covered_out /* host, Q */, rk_gather_stats *stats /* optional */);
/* Host only: the same rule over posting lists as rk_index_export_lists / rk_index_export64 return them (reference ids below n_ref in
 * any order within a list, repeats counted once) -- blind to the hash width: per query i the indices of the lists its hashes hit,
 * strictly ascending, are q_lists[q_off[i] .. q_off[i + 1]).  ref_sizes (n_ref) and query_sizes (n_query) only fill the records.  The
 * outputs are those of rk_gather_rows.  RK_ERR_ARG: null pointers (postings / counts may be NULL without lists, q_lists when no query
 * hits a list, the size arrays and the per-query outputs when their number is 0), min_new == 0, offsets that do not ascend from 0, a
 * list index >= n_lists or out of order, a posting >= n_ref.  Nothing is written on a refusal. */
int rk_gather_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, const uint64_t *q_off /* n_query + 1 */,
                    const uint64_t *q_lists, uint32_t n_query, uint32_t n_ref, const uint32_t *ref_sizes, const uint32_t *query_sizes,
                    const rk_gather_opts *opts, uint64_t *off_out /* n_query + 1 */, rk_gather_pick **picks_out, uint64_t *n_picks,
                    uint32_t *matched_out, uint32_t *n_cand_out, uint32_t *covered_out);

/* ---- filtering query sketches by an index ------------------------------------------------ */
/* rk_sketches_mask: every query sketch without (or with only) the hashes that the references of an index hold -- the reference's `sub`
 * ("subtract the reference sketch from the query sketches") and three relatives, on the device, in integers only.
 * For a query hash h, c(h) = the length of h's posting list in the index, 0 when it has none: a hash at or beyond 2^hash_bits of the
 * index has no list; a reference sketch that repeats a hash lengthens the list, exactly as it counts in rk_dist_rows; for set sketches
 * c(h) is the number of references that hold h.  h survives iff min_refs <= c(h) <= max_refs:
 *   {0, 0}            the reference's `sub`: the hashes no reference holds;
 *   {1, UINT32_MAX}   the intersection: the hashes at least one reference holds;
 *   {0, m}            without the hashes more than m references hold ("stop words");
 *   {m, UINT32_MAX}   only the hashes at least m references hold.
 * *out (library-owned, rk_sketches_free) has as many sketches as the queries, in their order, and their hash width; each holds its
 * surviving hashes in the order a device-resident sketch has them: ascending, repeats kept with their multiplicity.  A sketch that
 * loses everything stays, as an empty sketch.  The object is a sketches object like any other (rk_index_build, rk_dist_rows,
 * rk_dist_topn, rk_assign_rows, rk_gather_rows, rk_sketches_download / download64); rk_sketches_windows() of it is 0.
 * The result is unique: it does not depend on the internal genome order, on how the index came to be (built or imported) or on the leg.
 * On the device (rk_mask.hip), flat over all query hashes in tiles of tile_hashes, never one workgroup per sketch: the flag kernel looks
 * every hash up (the bucket of the prefix directory, then a binary search among the distinct hashes), applies the band to the length of
 * its list and writes one 64-bit keep word per 64 hashes and the tile's count; an exclusive scan of the tile counts (scan_blocks
 * blocks); the scatter kernel re-reads hashes and keep words and writes every survivor at tile prefix + kept bits before it (order
 * preserved, no atomics); the offsets kernel computes off_out[g] = the survivors before off_in[g] from the same words.  No kernel waits
 * for another workgroup.  One read-back brings the n + 1 offsets and the counters.
 * RK_MASK_DEVICE=0 answers inside the call as export + rk_mask_lists + rk_sketches_from_host(64), with the same result; stats->path
 * says which leg ran.
 * RK_ERR_ARG: null pointers, min_refs > max_refs, queries and index of different hash widths, an index without all posting lists (the
 * join-only index of rk_index_join_shard, one hash range of a sharded build).  Nothing is written on a refusal.  No query sketch:
 * RK_OK, *out = NULL, nothing runs.  An index without genomes or without hashes is legal: every c(h) is 0. */
#define RK_MS_MASK 15           /* rk_sketches_mask: the flag kernel through the offsets kernel of the last call; 0 on the host leg */
typedef struct rk_mask_rule {
    uint32_t min_refs, max_refs;   /* h survives iff min_refs <= c(h) <= max_refs */
} rk_mask_rule;                    /* 8 bytes */
typedef struct rk_mask_stats {
    uint64_t hashes, kept, matched;   /* query hashes in, out, and those with c(h) > 0 */
    uint64_t tiles;                   /* tiles of the flag / scatter kernels: ceil(hashes / tile_hashes) */
    uint32_t emptied;                 /* non-empty sketches that end empty */
    uint32_t path;                    /* 0 nothing ran, 1 the device, 2 the host (RK_MASK_DEVICE=0) */
    uint32_t tile_hashes, scan_blocks, threads;   /* hashes of a tile, blocks of the scan of the tile counts, threads of a workgroup:
                                                     constants / geometry, filled on every path that ran */
    uint32_t pad_;
} rk_mask_stats;                      /* 56 bytes */
int rk_sketches_mask(rk_ctx *ctx, const rk_sketches *queries, const rk_index *idx, const rk_mask_rule *rule, rk_sketches **out,
                     rk_mask_stats *stats /* optional */);
/* Host only, no context: the same rule over the distinct hashes and list lengths as rk_index_export_lists / rk_index_export64 return them
 * (list_hashes strictly ascending: uint32 when wide == 0, uint64 otherwise, like q_hashes).  The hashes of query i are
 * q_hashes[q_off[i] .. q_off[i + 1]), in ANY order; the survivors keep their order.  *hashes_out (rk_free_host; NULL when nothing
 * survives) holds them back to back, off_out (caller's, n_query + 1) delimits them.  stats (optional): hashes, kept, matched, emptied.
 * RK_ERR_ARG: null pointers (q_hashes may be NULL without hashes, list_hashes / counts without lists), min_refs > max_refs, offsets
 * that do not ascend from 0, list hashes that do not strictly ascend.  Nothing is written on a refusal. */
int rk_mask_lists(const void *q_hashes, int wide, const uint64_t *q_off /* n_query + 1 */, uint32_t n_query, const void *list_hashes,
                  const uint32_t *counts, uint64_t n_lists, const rk_mask_rule *rule, void **hashes_out, uint64_t *off_out /* n_query + 1 */,
                  rk_mask_stats *stats /* optional */);

/* rk_sketches_mask_counts: rk_sketches_mask for COUNTED queries (rk_sketches_has_counts; RK_ERR_UNSUPPORTED without counts, nothing
 * written).  The rule, the statistics, the hashes and the offsets are those of rk_sketches_mask, byte for byte; *out carries counts:
 * every surviving hash keeps its count (the scatter kernel in a second instantiation writes it beside the hash).  RK_MASK_DEVICE=0
 * answers inside the call as export + rk_mask_lists_counts + rk_sketches_from_host_counts.  rk_mask_lists_counts: rk_mask_lists with
 * q_counts parallel to q_hashes (RK_ERR_ARG when NULL with hashes) and *counts_out (rk_free_host; NULL when nothing survives)
 * parallel to *hashes_out. */
int rk_sketches_mask_counts(rk_ctx *ctx, const rk_sketches *queries, const rk_index *idx, const rk_mask_rule *rule, rk_sketches **out,
                            rk_mask_stats *stats /* optional */);
int rk_mask_lists_counts(const void *q_hashes, const uint32_t *q_counts, int wide, const uint64_t *q_off /* n_query + 1 */, uint32_t n_query,
                         const void *list_hashes, const uint32_t *counts, uint64_t n_lists, const rk_mask_rule *rule, void **hashes_out,
                         uint32_t **counts_out, uint64_t *off_out /* n_query + 1 */, rk_mask_stats *stats /* optional */);

/* ---- taxonomic classification by per-hash LCA -------------------------------------------- */
/* rk_lca_rows: per query sketch the tally of the lowest common ancestors of its hashes in a taxonomy over the references -- the rule of
 * Kraken and of sourmash `lca classify` / `summarize`, on the device, in integers only.
 * Taxonomy: parent[0 .. n_taxa) (host); parent[t] == t marks the root, of which there is exactly one; every other node reaches it by
 * following parent.  Node ids are the caller's: no order, no depth bound.  taxa[0 .. N) (host) names the node of every reference in the
 * CALLER's genome order, RK_LCA_NONE leaves a reference unlabelled.
 * Per hash h with a posting list: lca(h) = the lowest common ancestor of the taxa of its labelled holders (a genome that repeats h is a
 * holder like any other; an unlabelled holder is ignored -- unlike rk_group_sketches `only`, where it defeats the hash); undefined when
 * no holder is labelled.
 * Per selected query row q (row_first / row_step / row_block as in rk_gather_opts), every ELEMENT of the sketch counting, a repeated
 * hash as often as it occurs (as in rk_sketches_mask):
 *   matched[q]      the elements with a posting list (a hash at or beyond 2^hash_bits of the index has none);
 *   unlabelled[q]   the matched elements whose lca is undefined;
 *   the tally       the records {taxon, direct} with direct > 0 = the matched elements with lca == taxon, by ascending caller node id:
 *                   (*counts_out)[off_out[q] .. off_out[q + 1]).  sum(direct) + unlabelled[q] == matched[q].
 * off_out (host, Q + 1) is written in full (an unselected row is empty); *counts_out is the library's (rk_free_host; NULL when there is
 * no record); matched_out / unlabelled_out (host, Q entries each): only the entries of the selected rows are written.  The result is
 * unique: it does not depend on the internal genome order, on how the index came to be (built or imported), on how the nodes are
 * numbered (the records map onto each other), on tiles, shards or the leg.  A row depends on its own elements alone: row shards
 * concatenate, no merge call is needed.
 * Accepted: every index that carries all posting lists, built or imported.  Traffic: 16 * n_taxa + 4 * N bytes go up; the counters,
 * 8 * (Q + 1) bytes of offsets, 8 * Q bytes of the two per-row counts and 8 bytes per record come back, never a hash, a posting or the
 * taxon of a list.
 * On the device (rk_lca.hip), one stream: the host validates the taxonomy and numbers it in preorder (iterative, children by ascending
 * id); the preorder id of every genome's taxon in internal genome order; per posting list the smallest and the largest preorder id of
 * its labelled postings -- the LCA of a set is the LCA of these two -- and one climb from the smaller, by list length: one lane up to
 * lane_max postings, one wave up to wave_max, a workgroup that streams chunks of `chunk` postings beyond; then flat over all query
 * elements in tiles of tile_hashes, never one workgroup per sketch: the look-up (the bucket of the prefix directory, a binary search),
 * the row of the element (a binary search among the query offsets), a tile-local table of table_slots slots in LDS keyed by
 * row << 32 | taxon, one reservation per tile for its partial records; these sorted, equal keys summed, offsets taken.  No kernel
 * waits for another workgroup.  When the partial records outgrow their buffer the query pass runs once more with the exact count
 * (attempts = 2).  The host synchronises for the counters, for the offsets and per-row counts, and for the records.
 * RK_LCA_DEVICE=0 answers inside the call as export + look-up + rk_lca_lists, with the same result; stats->path says which leg ran.
 * RK_ERR_ARG: null pointers, n_taxa == 0, no root or two, a parent >= n_taxa, a cycle, a taxon that is neither < n_taxa nor
 * RK_LCA_NONE, queries and index of different hash widths, an index without all posting lists (the join-only index of
 * rk_index_join_shard, one hash range of a sharded build).  RK_ERR_UNSUPPORTED: n_taxa or N at 2^31 or more, a query sketch of 2^32
 * elements or more.  Nothing is written on a refusal.  No query sketch: RK_OK, nothing runs.  An index without genomes, without hashes
 * or without a labelled genome is legal: every tally is empty, matched is still counted. */
#define RK_LCA_NONE 0xFFFFFFFFu /* taxa[]: an unlabelled reference; rk_lca_called: no call */
#define RK_MS_LCA 16            /* rk_lca_rows: k_lca_taxa through the fold of the last call; 0 on the host leg */
typedef struct rk_lca_opts {
    uint32_t row_first, row_step, row_block;   /* the row shard, as in rk_gather_opts (0 0 0: every query) */
} rk_lca_opts;                  /* 12 bytes */
typedef struct rk_lca_count {
    uint32_t taxon, direct;     /* the caller's node id; the matched elements of the query whose lca is this node (> 0) */
} rk_lca_count;                 /* 8 bytes */
typedef struct rk_lca_rule {
    uint32_t min_count;         /* >= 1: a record counts from this many elements on */
    uint32_t conf_num, conf_den;   /* the confidence conf_num / conf_den in [0, 1]: conf_num <= conf_den, conf_den >= 1 */
    uint32_t denom;             /* the denominator of the confidence: 0 the retained elements, 1 the size of the query sketch */
} rk_lca_rule;                  /* 16 bytes */
typedef struct rk_lca_called {
    uint32_t taxon;             /* the call, RK_LCA_NONE when the root fails too or nothing is retained */
    uint32_t candidate;         /* the LCA of the retained nodes of maximal score (RK_LCA_NONE: nothing retained) */
    uint32_t clade;             /* clade(taxon); clade(root) when there is no call */
    uint32_t score;             /* the maximal score */
    uint32_t retained;          /* the sum of direct over the retained records */
    uint32_t n_taxa;            /* the retained records */
} rk_lca_called;                /* 24 bytes */
typedef struct rk_lca_stats {
    uint64_t lists, postings;   /* posting lists and postings of the index */
    uint64_t lane_lists, wave_lists, block_lists;   /* lists by the class of their length (lane_max, wave_max) */
    uint64_t elements;          /* query elements of the selected rows */
    uint64_t matched, unlabelled, records;   /* summed over the selected rows */
    uint64_t partials;          /* (row, taxon, count) records the tiles emitted (device leg) */
    uint64_t tiles;             /* tiles of the query pass: ceil(all query elements / tile_hashes) */
    uint32_t longest_climb;     /* the most parent steps one list took from its smallest preorder id to its lca (device leg) */
    uint32_t path;              /* 0 nothing ran, 1 the device, 2 the host (RK_LCA_DEVICE=0, rk_lca_lists) */
    uint32_t attempts;          /* runs of the query pass: 2 after an overflow of the partial records */
    uint32_t rows;              /* selected rows */
    uint32_t lane_max, wave_max, chunk, tile_hashes, table_slots, threads;   /* constants, filled on every path that ran */
} rk_lca_stats;                 /* 128 bytes */
int rk_lca_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const uint32_t *taxa /* N */, const uint32_t *parent /* n_taxa */,
                uint32_t n_taxa, const rk_lca_opts *opts, uint64_t *off_out /* Q + 1 */, rk_lca_count **counts_out, uint64_t *n_counts,
                uint32_t *matched_out /* Q */, uint32_t *unlabelled_out /* Q */, rk_lca_stats *stats /* optional */);
/* Host only, no context: the same rule over posting lists as rk_index_export_lists / rk_index_export64 return them (reference ids below
 * n_ref in any order within a list, a repeated id a holder like any other) -- blind to the hash width: per query i the indices of the
 * lists its elements hit, ascending, repeats allowed, one per matched element, are q_lists[q_off[i] .. q_off[i + 1]).  The LCA of a
 * list is folded pairwise by depth and parent steps; nothing is numbered in preorder: the two legs do not share their algorithm.  The
 * outputs are those of rk_lca_rows.  RK_ERR_ARG: null pointers (postings / counts may be NULL without lists, q_lists when no element hits
 * a list, taxa when n_ref is 0, the per-query outputs when n_query is 0), a bad taxonomy or taxon as above, offsets that do not ascend
 * from 0, a list index >= n_lists or out of order, a posting >= n_ref.  RK_ERR_UNSUPPORTED as above.  Nothing is written on a refusal. */
int rk_lca_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, const uint64_t *q_off /* n_query + 1 */,
                 const uint64_t *q_lists, uint32_t n_query, uint32_t n_ref, const uint32_t *taxa /* n_ref */, const uint32_t *parent /* n_taxa */,
                 uint32_t n_taxa, const rk_lca_opts *opts, uint64_t *off_out /* n_query + 1 */, rk_lca_count **counts_out, uint64_t *n_counts,
                 uint32_t *matched_out, uint32_t *unlabelled_out, rk_lca_stats *stats /* optional */);
/* Host only, no context: the call on the tally of every query (counts[off[q] .. off[q + 1]), as rk_lca_rows returns them; any order
 * within a query, every taxon at most once), the taxonomy and a rule.
 *   retained    the records with direct >= min_count; `retained` = the sum of their direct;
 *   clade(t)    the sum of retained direct over the subtree of t;  score(t) the sum over the path from the root to t;
 *   candidate   the LCA of the retained nodes of maximal score (Kraken's root-to-leaf rule with its tie rule);
 *   climb       from the candidate to the parent while clade(t) * conf_den < conf_num * D, D = retained (denom 0) or query_sizes[q]
 *               (denom 1); the first node that passes is the call; RK_LCA_NONE when the root fails too or nothing is retained.
 * {m, 1, 1, 0} is sourmash `lca classify --threshold m` (the LCA of every retained taxon), {1, 0, 1, *} Kraken without confidence.
 * called_out (host, n_query records); clade_out (optional, host, off[n_query] entries): clade(taxon) of every tally record, parallel
 * to counts.  RK_ERR_ARG: null pointers (counts may be NULL without records, query_sizes unless denom is 1), a bad taxonomy,
 * a record's taxon >= n_taxa or twice in a query, offsets that do not ascend from 0, min_count == 0, conf_den == 0, conf_num > conf_den,
 * denom > 1.  RK_ERR_UNSUPPORTED: a query whose direct counts add up to 2^32 or more (clade, score and retained are 32 bits wide; a
 * tally of rk_lca_rows cannot).  Nothing is written on a refusal. */
int rk_lca_call(const rk_lca_count *counts, const uint64_t *off /* n_query + 1 */, uint32_t n_query, const uint32_t *query_sizes /* n_query */,
                const uint32_t *parent /* n_taxa */, uint32_t n_taxa, const rk_lca_rule *rule, rk_lca_called *called_out /* n_query */,
                uint32_t *clade_out /* optional */);

/* ---- winner-take-all containment screen ---------------------------------------------------- */
/* rk_screen_rows: which references are contained in a query sketch, and how much of each survives once every shared hash is credited to
 * one reference only -- the question of `mash screen -w`, answered in one pass, in integers only.  Sketches are taken as SETS: an index
 * whose references repeat a hash and queries that repeat a hash are RK_ERR_UNSUPPORTED, as in rk_gather_rows.
 * Per selected query row q (row_first / row_step / row_block as in rk_gather_opts) with hash set S: matched[q] = the hashes of S that
 * have a posting list; common(r) = |S n R_r|; size(r) = |R_r|; the candidates = the references with common(r) >= min_common
 * (min_common >= 1); n_cand[q] = their number.  The candidates of a row are totally ordered: a is BETTER than b when, tested in this order,
 *   1. common(a) * size(b) > common(b) * size(a): the larger containment of the reference in the query, which is monotone in Mash's
 *      screen identity -- compared on 64-bit products, exact because every size is below 2^30;
 *   2. the products are equal and size(a) > size(b): Mash's tie rule, the larger reference;
 *   3. the sizes are equal too and the CALLER's index of a is smaller than that of b.
 * A matched hash is CLAIMED by the best candidate among its holders, by nobody when no holder is a candidate.  won(r) = the hashes r
 * claims; claimed[q] = the sum of won <= matched[q].  One record {query, ref, common, won, size_ref, size_query} per candidate with
 * won(r) >= min_won (0: every candidate), in (query, ascending CALLER's reference index) order: the records of query q are
 * (*recs_out)[off_out[q] .. off_out[q + 1]).  off_out (host, Q + 1 entries, every one written; an unselected row is empty);
 * *recs_out is the library's (rk_free_host; NULL when there is no record); matched_out / n_cand_out / claimed_out (host, Q entries
 * each): only the entries of the selected rows are written.
 * The result is unique: it does not depend on the internal genome order, on how the index came to be (built or imported), on batches,
 * on row shards or on the leg that ran.  A row depends on its own hashes alone: row shards concatenate, no merge call is needed.
 * With min_common = 1, claimed == matched.  The best candidate of a row has won == common.  A candidate whose hashes within S are a
 * subset of a better candidate's has won == 0.  common equals the count of rk_dist_rows for the pair.  When all references have one size,
 * the best candidate is the rank-0 pick of rk_gather_rows and its won that pick's fresh.
 * On the device (rk_screen.hip), one stream, per batch of query rows whose state fits RK_SCREEN_BATCH_BYTES (default 1 GiB; at least one
 * row; a row costs 8 N bytes: its counter row and its won row): the counter rows of the query join (stage A of rk_dist_topn), columns in
 * the caller's order; the winner pass, flat over all query hashes of the batch in tiles of tile_hashes, never one workgroup per sketch:
 * the look-up (the bucket of the prefix directory, a binary search), then the walk of the hash's posting list -- by the lane that found
 * it up to lane_max postings, by its wave up to wave_max (64 postings per trip, a wave reduction of the best key), by the workgroup
 * beyond (an LDS queue) -- comparing (common, size, caller's index) of every posting that is a candidate; the winner takes +1 on
 * won[row][ref] (a relaxed agent-scope integer add; equal (row, winner) of a wave are combined first, RK_SCREEN_COMBINE=0: lane by
 * lane).  Then a count kernel (candidates, records and the sum of won per row), a scan over the rows, ONE read-back for the room, and a
 * write kernel, one workgroup per row taking the row in chunks with a block scan: the records come out in ascending caller's index
 * without atomics and without a sort.  No kernel waits for another workgroup.  One copy carries 24 records + 12 Q + 8 (Q + 1) bytes;
 * counter rows and postings never leave the device.
 * RK_SCREEN_DEVICE=0 answers inside the call as export + rk_screen_lists, with the same result; stats->path says which leg ran.
 * RK_ERR_ARG: null pointers, min_common == 0, an index without posting lists (the join-only index of rk_index_join_shard, one hash range
 * of a sharded build), queries and index of different hash widths.  RK_ERR_UNSUPPORTED: sketches that repeat a hash, an index of
 * 2^31 - 1 postings or more, a sketch of 2^30 hashes or more (the products).  Nothing is written on a refusal.  No query: RK_OK, nothing
 * runs.  An index without genomes: RK_OK, every row empty. */
#define RK_MS_SCREEN 17         /* rk_screen_rows: the counts of the first batch through the last write kernel; 0 on the host leg */
typedef struct rk_screen_opts {
    uint32_t min_common;     /* >= 1: a candidate shares at least this many hashes with the query */
    uint32_t min_won;        /* a record is written for a candidate that claims at least this many hashes; 0: every candidate */
    uint32_t row_first, row_step, row_block;   /* the row shard, as in rk_gather_opts (0 0 0: every query) */
} rk_screen_opts;            /* 20 bytes */
typedef struct rk_screen_rec {
    uint32_t query, ref;     /* the query row and the CALLER's reference index */
    uint32_t common;         /* |S n R_ref| */
    uint32_t won;            /* the hashes of the query that ref claims */
    uint32_t size_ref, size_query;
} rk_screen_rec;             /* 24 bytes */
typedef struct rk_screen_stats {
    uint64_t records, candidates, matched, claimed;   /* sums over the selected rows */
    uint64_t postings_walked;   /* postings of the matched lists of the selected rows */
    uint64_t adds;              /* atomic adds on the won rows, after any combine (device leg) */
    uint64_t lane_lists, wave_lists, block_lists;   /* matched lists by who walks them (the host leg: by the class of their length) */
    uint64_t rows_per_batch;
    uint32_t path;           /* 0 nothing ran, 1 the device, 2 the host (RK_SCREEN_DEVICE=0) */
    uint32_t rows;           /* selected rows */
    uint32_t batches;
    uint32_t launches;       /* kernels of this unit the host launched */
    uint32_t read_backs;     /* synchronising reads of the counters: one per batch */
    uint32_t lane_max, wave_max, tile_hashes, threads;   /* the constants of the winner pass (every path fills them) */
    uint32_t pad_;
} rk_screen_stats;           /* 120 bytes */
int rk_screen_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_screen_opts *opts, uint64_t *off_out /* host, Q + 1 */,
                   rk_screen_rec **recs_out, uint64_t *n_recs, uint32_t *matched_out /* host, Q */, uint32_t *n_cand_out /* host, Q */,
                   uint32_t *claimed_out /* host, Q */, rk_screen_stats *stats /* optional */);
/* Host only, no context: the same rule over posting lists as rk_index_export_lists / rk_index_export64 return them (reference ids below
 * n_ref in any order within a list, repeats counted once) -- blind to the hash width: per query i the indices of the lists its hashes
 * hit, strictly ascending, are q_lists[q_off[i] .. q_off[i + 1]).  ref_sizes (n_ref) is part of the rule; query_sizes (n_query) only
 * fills the records.  The outputs are those of rk_screen_rows.  RK_ERR_ARG: null pointers (postings / counts may be NULL without lists,
 * q_lists when no query hits a list, the size arrays and the per-query outputs when their number is 0), min_common == 0, offsets that do
 * not ascend from 0, a list index >= n_lists or out of order, a posting >= n_ref, a size of 2^30 or more, a reference of a selected row
 * whose common exceeds its ref_sizes entry.  Nothing is written on a refusal. */
int rk_screen_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, const uint64_t *q_off /* n_query + 1 */,
                    const uint64_t *q_lists, uint32_t n_query, uint32_t n_ref, const uint32_t *ref_sizes, const uint32_t *query_sizes,
                    const rk_screen_opts *opts, uint64_t *off_out /* n_query + 1 */, rk_screen_rec **recs_out, uint64_t *n_recs,
                    uint32_t *matched_out, uint32_t *n_cand_out, uint32_t *claimed_out);

/* ---- the screen with abundances ------------------------------------------------------------------ */
/* rk_screen_abund_rows: rk_screen_rows for COUNTED query sketches (rk_sketches_has_counts; RK_ERR_UNSUPPORTED without counts, nothing
 * written).  The rule does not change: off_out, *recs_out, *n_recs, matched_out, n_cand_out and claimed_out are byte for byte those of
 * rk_screen_rows for the same index, queries and options.  With m(h) >= 1 the count of hash h in its query, every record gets a parallel
 * record (*abund_out)[i] (the library's, rk_free_host; NULL when there is no record):
 *   occ_common  the sum of m(h) over S n R_ref          med_common  the LOWER median of m(h) over S n R_ref
 *   occ_won     the sum of m(h) over the hashes ref claims   med_won  the lower median over the claimed hashes, 0 when won == 0
 * The lower median of n values is the one of 0-based rank (n - 1) / 2 in ascending order.  occ_out (host, 3 Q entries; only those of the
 * selected rows are written): occ_out[3 q] = the sum of m over the whole sketch q, [3 q + 1] over its matched hashes, [3 q + 2] over its
 * claimed hashes.  Everything is integers; the result is unique as that of rk_screen_rows is, and row shards concatenate.
 * On the device the batches, the counter rows, the winner pass, the count, the scan and the write are those of rk_screen_rows (the count
 * and the write kernel in a second instantiation: the one read-back of a batch also brings every row's records and the sum of their
 * common, the write also leaves, in the dead won row, the record of every cell + 1 and gives every record a segment of exactly `common`
 * values).  Then, per sub-range of the batch's rows whose values fit RK_SCREEN_VALUE_BYTES (default: the batch budget; at least one
 * row), nothing read back in between: the fill kernel -- the tiles, the look-up and the three walks of the winner pass; it finds the
 * winner of a hash again (one more walk of a list that is in cache, instead of 4 bytes per query hash and another instantiation of
 * the winner kernel) and hands m(h) to every holder with a record, the winner's at seg + front++, the others' at seg + common - 1 -
 * back++ (relaxed agent-scope adds on two cursors per record), so a segment holds its claimed values in [0, won) -- and the select
 * kernels: a segment of up to rank_max values is ranked by one wave in registers, one of up to wave_sel_max by one wave with a radix
 * select (four rounds of a pair of 256-bin LDS histograms: the claimed part and the whole together), a longer one by a workgroup.
 * Nothing is sorted, no kernel waits for another workgroup, every store is a plain vector store.
 * RK_SCREEN_DEVICE=0 answers inside the call as export + rk_screen_abund_lists, with the same bytes; stats->path says which leg ran.
 * The refusals and the empty cases are those of rk_screen_rows; abund_out and occ_out (Q > 0) must not be NULL. */
#define RK_MS_SCREEN_ABUND 18   /* rk_screen_abund_rows: the counts of the first batch through the last select kernel; 0 on the host leg */
typedef struct rk_screen_abund {
    uint64_t occ_common;     /* the sum of m(h) over S n R_ref */
    uint64_t occ_won;        /* the sum of m(h) over the hashes ref claims */
    uint32_t med_common;     /* the lower median of m(h) over S n R_ref */
    uint32_t med_won;        /* the lower median over the claimed hashes; 0 when won == 0 */
} rk_screen_abund;           /* 24 bytes */
typedef struct rk_screen_abund_stats {
    uint64_t records, candidates, matched, claimed;   /* these 120 bytes: rk_screen_stats, field by field */
    uint64_t postings_walked;
    uint64_t adds;
    uint64_t lane_lists, wave_lists, block_lists;
    uint64_t rows_per_batch;
    uint32_t path;
    uint32_t rows;
    uint32_t batches;
    uint32_t launches;
    uint32_t read_backs;
    uint32_t lane_max, wave_max, tile_hashes, threads;
    uint32_t pad_;
    uint64_t values;         /* the sum of common over the records: the values handed out */
    uint64_t value_bytes;    /* the budget of the values of one sub-range (device leg) */
    uint64_t rank_segs, wave_segs, block_segs;   /* records by who selects their medians (the host leg: by the class of their length) */
    uint32_t value_passes;   /* fill passes: the sub-ranges of all batches (device leg) */
    uint32_t rank_max, wave_sel_max, chunk;   /* a wave ranks up to rank_max values in registers, selects up to wave_sel_max by radix; a
                                                 workgroup takes longer segments, `chunk` values per step (every path fills them) */
} rk_screen_abund_stats;     /* 176 bytes */
int rk_screen_abund_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_screen_opts *opts, uint64_t *off_out /* host, Q + 1 */,
                         rk_screen_rec **recs_out, rk_screen_abund **abund_out, uint64_t *n_recs, uint32_t *matched_out /* host, Q */,
                         uint32_t *n_cand_out /* host, Q */, uint32_t *claimed_out /* host, Q */, uint64_t *occ_out /* host, 3 Q */,
                         rk_screen_abund_stats *stats /* optional */);
/* Host only, no context: rk_screen_lists with q_counts parallel to q_lists (the count of the query hash that hit that list, >= 1) and
 * query_occ (n_query: the sum of the counts of the whole sketch, which only fills occ_out[3 q]).  RK_ERR_ARG: what rk_screen_lists
 * refuses, abund_out or occ_out (n_query > 0) NULL, q_counts NULL when a query hits a list, query_occ NULL when n_query > 0, a count of
 * 0.  Nothing is written on a refusal. */
int rk_screen_abund_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, const uint64_t *q_off /* n_query + 1 */,
                          const uint64_t *q_lists, const uint32_t *q_counts, uint32_t n_query, uint32_t n_ref, const uint32_t *ref_sizes,
                          const uint32_t *query_sizes, const uint64_t *query_occ, const rk_screen_opts *opts, uint64_t *off_out /* n_query + 1 */,
                          rk_screen_rec **recs_out, rk_screen_abund **abund_out, uint64_t *n_recs, uint32_t *matched_out, uint32_t *n_cand_out,
                          uint32_t *claimed_out, uint64_t *occ_out /* 3 n_query */);

/* one output line, "%s\t%s\t%d|%d|%d\t%f\t%f\n" (src/dist.cpp:233 / :642) */
int rk_format_hit(char *buf, size_t cap, const char *name_a, const char *name_b,
                  const rk_hit *hit);

#ifdef __cplusplus
}
#endif
#endif /* RABBITKSSD_H */
