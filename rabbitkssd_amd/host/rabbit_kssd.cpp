// rabbit_kssd.cpp -- host tool with RabbitKSSD's command line (src/main.cpp:34-145) for the
// hot-path subcommands, built on the C ABI of librabbitkssd.so (include/rabbitkssd.h).
//
//   shuffle  -k -s -l -o                     (host only, src/shuffle.cpp:25-104)
//   sketch   -i list -o out [-L shuf] [-q] [-Q q -n c]   (GPU: rk_sketch_batch_ex [+ rk_index_build];
//                                             FASTA or FASTQ lists, plain or .gz)
//   alldist  -i sketch|list -o out [-D -M -L]            (GPU: rk_index_build, rk_dist_rows)
//   dist     -r ref -q qry -o out [-D -M -N -L]          (GPU: rk_dist_rows; -N: rk_dist_topn)
//   sketch   ... --abund                     (the counted calls: also <out>.sketch.abund, the occurrence count of every kept hash)
//   abund    -i sketch [-o out] [--bins B] | --min-count N [--max-count M] -o out.sketch   (host only: report / band of counts)
//   info     -i sketch -o out [-F]           (host only, src/subCommand.cpp:70-147)
//   merge    -i list -o out                  (host only, src/subCommand.cpp:796-892)
//   union / sub                              (host only, src/subCommand.cpp:307-794)
//   convert [--reverse]                      (host formats, src/sketch.cpp:1179-1365; index on GPU)
// Errors follow the reference: a message on stderr and exit(1).  There is no CPU fallback:
// without a GPU the GPU subcommands fail at rk_ctx_create.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <iostream>
#include <map>
#include <memory>
#include <thread>

#include "formats.hpp"
#include "sketch_input.hpp"
#include "rabbitkssd.h"

using namespace rkhost;
using std::cerr;
using std::endl;
using std::string;
using std::vector;

static double get_sec()
{
    struct timeval tv;
    gettimeofday(&tv, nullptr);
    return (double)tv.tv_sec + (double)tv.tv_usec / 1e6;
}

[[noreturn]] static void die(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "ERROR: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}

static const double g_t_start = get_sec();
static void stamp(const char *what)
{
    static const bool on = getenv("RK_TIMING") != nullptr;
    if (on) fprintf(stderr, "[timing] %8.3f ms  %s\n", (get_sec() - g_t_start) * 1e3, what);
}

struct Gpu {
    rk_ctx *ctx = nullptr;
    explicit Gpu(int device)
    {
        stamp("before rk_ctx_create");
        int rc = rk_ctx_create(device, &ctx);
        if (rc) die("no usable GPU (rk_ctx_create(%d) = %d): this build has no CPU path", device, rc);
        rk_ctx_set_single_shot(ctx, 1);   // one pass per process: nothing amortises a one-time device-side setup
        stamp("context ready");
    }
    // The process ends right after its last GPU call (main leaves through _exit): returning ~600 MB of pooled device
    // memory block by block and tearing the HIP runtime down costs 60-100 ms that buy nothing.
    ~Gpu() {}
    void check(int rc, const char *what) const
    {
        if (rc) die("%s failed (%d): %s", what, rc, rk_last_error(ctx));
    }
};

// HIP runtime start-up (hipInit: 150-190 ms on an MI355X box) is the largest single item of a short alldist/dist run:
// it starts on a thread of its own while the main thread reads the .sketch files
struct AsyncGpu {
    std::unique_ptr<Gpu> g;
    std::thread th;
    explicit AsyncGpu(int device) : th([this, device] { g.reset(new Gpu(device)); }) {}
    Gpu &get()
    {
        if (th.joinable()) th.join();
        return *g;
    }
    ~AsyncGpu() { if (th.joinable()) th.join(); }
};

// ---- tiny option parser -----------------------------------------------------------------
struct Args {
    std::map<string, string> kv;
    std::map<string, bool> seen;
    bool has(const string &k) const { return seen.count(k) != 0; }
    string str(const string &k, const string &d) const { auto it = kv.find(k); return it == kv.end() ? d : it->second; }
    int num(const string &k, int d) const { auto it = kv.find(k); return it == kv.end() ? d : atoi(it->second.c_str()); }
    double real(const string &k, double d) const { auto it = kv.find(k); return it == kv.end() ? d : atof(it->second.c_str()); }
};

// spec: {"-k","--halfk"} -> canonical "k"; flags take no value
static Args parse_args(int argc, char **argv, int first, const std::map<string, string> &alias,
                       const std::vector<string> &flags)
{
    Args a;
    for (int i = first; i < argc; i++) {
        string t = argv[i], val;
        bool has_val = false;
        auto eq = t.find('=');
        if (t.rfind("--", 0) == 0 && eq != string::npos) { val = t.substr(eq + 1); t = t.substr(0, eq); has_val = true; }
        auto it = alias.find(t);
        if (it == alias.end()) die("unknown option %s", argv[i]);
        const string key = it->second;
        a.seen[key] = true;
        if (std::find(flags.begin(), flags.end(), key) != flags.end()) { a.kv[key] = "1"; continue; }
        if (!has_val) {
            if (i + 1 >= argc) die("option %s needs a value", argv[i]);
            val = argv[++i];
        }
        a.kv[key] = val;
    }
    return a;
}

// ---- sketching --------------------------------------------------------------------------
// Replaces sketchFastaFile (src/sketch.cpp:318-593): genomes keep list order and hashes are
// sorted (the reference's order is unordered_set / OpenMP completion order; every consumer
// treats them as sets).
struct FastqOpts {
    bool fastq = false;   // the list holds FASTQ files (sketchFastqFile, src/sketch.cpp:596-890)
    int least_qual = 0;   // -Q
    int least_num = 1;    // -n
};

// '>' -> FASTA list, '@' -> FASTQ list, anything else / mixed -> error (src/sketch.cpp:52-94,
// src/subCommand.cpp:54-62).  *.gz names are accepted by suffix like isFastaGZList/isFastqGZList.
static bool list_is_fastq(const vector<string> &files)
{
    int n_fa = 0, n_fq = 0;
    for (const string &f : files) {
        int c;
        if (ends_with(f, ".gz")) c = (ends_with(f, ".fq.gz") || ends_with(f, ".fastq.gz")) ? '@' : '>';
        else c = first_byte(f);
        if (c == '>') n_fa++;
        else if (c == '@') n_fq++;
        else die("the input file list for sketching must be list of fasta and fastq file in normal format or gz format");
    }
    if (n_fa && n_fq) die("the input file list for sketching must be list of fasta and fastq file in normal format or gz format");
    return n_fq > 0;
}

// ---- streaming pipeline (the role of src/sketch.cpp:318-460's producer/consumer threads) ----
// Files are grouped into batches that fit one page-locked staging buffer (the plan: sketch_input.hpp).  The parser
// threads write every genome straight into its 1 KiB-aligned slot of the staging buffer in the packed layout of
// rk_sketch_packed_dev (no intermediate copy); a GPU thread uploads the batch, runs the sketch kernels and downloads the
// hashes while the parser threads already fill the other staging buffer.  A file bigger than the staging buffer gets a
// batch of its own and is streamed piece by piece (sketch_streamed), or, with RK_BIG_WHOLE or where the streamed
// readers decline, parsed whole into ordinary memory.
struct ListSketcher {
    Gpu &gpu;
    const rk_filter *flt;
    const vector<string> &files;
    const Shuf &shuf;
    const int threads;
    const FastqOpts &fq;
    SketchSet &out;
    const bool abund;   // --abund: every sketch call is the counted one, out.counts follows out.hashes
    const bool timing = getenv("RK_TIMING") != nullptr;
    uint64_t total_windows = 0;

    // the plan
    uint64_t stage_bytes = 0, dev_bytes = 0;
    vector<Batch> batches;
    // the buffers
    int n_buf = 0;
    uint8_t *stage[2] = {nullptr, nullptr};
    void *dev[2] = {nullptr, nullptr};
    void *stream = nullptr;
    RawBuf big_stage;  // pageable staging of an oversized file
    // hand-over of filled staging buffers to the GPU thread: (batch, buffer), in list order; buffer b is stage[b] and dev[b]
    // (two slots also where a single batch has n_buf == 1: slots come out in order, and one batch only ever takes slot 0)
    PieceRing<size_t> staging{2, 1};

    uint32_t min_count() const { return (uint32_t)std::max(1, fq.least_num); }
    // the packed sketch call of this job: the counted one with --abund (the same arguments)
    decltype(&rk_sketch_packed_dev_ex) packed_call() const { return abund ? rk_sketch_packed_dev_counts : rk_sketch_packed_dev_ex; }
    const char *packed_name() const { return abund ? "rk_sketch_packed_dev_counts" : "rk_sketch_packed_dev_ex"; }

    void plan()
    {
        vector<uint64_t> bound(files.size());
        uint64_t total_bound = 0, max_bound = 0;
        for (size_t i = 0; i < files.size(); i++) {
            uint64_t packed = 0;
            if (!packed_bound(files[i], packed)) die("cannot open the genome file: %s", files[i].c_str());
            bound[i] = slot_bound(packed);
            total_bound += bound[i];
            max_bound = std::max(max_bound, bound[i]);
        }
        stage_bytes = stage_size(total_bound);
        dev_bytes = std::max(stage_bytes, max_bound);
        batches = plan_batches(bound, stage_bytes);
    }

    void alloc_buffers()
    {
        const double t_alloc = get_sec();
        n_buf = batches.size() > 1 ? 2 : 1;
        gpu.check(rk_stream_create(gpu.ctx, &stream), "rk_stream_create");
        bool need_pinned = false;
        for (const Batch &bt : batches) need_pinned |= !bt.pageable;
        for (int k = 0; k < n_buf; k++) {
            if (need_pinned) gpu.check(rk_pinned_alloc(gpu.ctx, stage_bytes, (void **)&stage[k]), "rk_pinned_alloc");
            gpu.check(rk_dev_alloc(gpu.ctx, dev_bytes, &dev[k]), "rk_dev_alloc");
        }
        if (timing) fprintf(stderr, "[timing] %d staging buffer(s) of %.1f MB pinned + device: %.3f s\n", n_buf, stage_bytes / 1e6, get_sec() - t_alloc);
    }
    void free_buffers()
    {
        // the page-locked buffers go back to the system while the sketches are saved and the index is built (unpinning is
        // kernel work that needs nothing from this thread)
        const double t_free = get_sec();
        for (int k = 0; k < n_buf; k++) rk_dev_free(dev[k]);
        rk_stream_destroy(stream);
        // (detached: the GPU subcommands leave through _exit once their output is on disk)
        std::thread([st0 = stage[0], st1 = stage[1], timing = timing, t_free] {
            rk_pinned_free(st0);
            rk_pinned_free(st1);
            if (timing) fprintf(stderr, "[timing] staging buffers released (in the background): %.3f s\n", get_sec() - t_free);
        }).detach();
    }

    // ---- results: a sketches object of n genomes into (hashes, offsets), once for both hash widths
    SketchSet download(rk_sketches *sk, uint32_t n)
    {
        SketchSet d;
        d.off.resize((size_t)n + 1);
        if (out.wide()) {
            d.hashes64.resize(rk_sketches_total(sk));
            gpu.check(rk_sketches_download64(sk, d.hashes64.data(), d.off.data()), "rk_sketches_download64");
        } else {
            d.hashes.resize(rk_sketches_total(sk));
            gpu.check(rk_sketches_download(sk, d.hashes.data(), d.off.data()), "rk_sketches_download");
        }
        if (abund) {
            d.counts.resize(rk_sketches_total(sk));
            if (!d.counts.empty()) gpu.check(rk_sketches_download_counts(sk, d.counts.data()), "rk_sketches_download_counts");
        }
        total_windows += rk_sketches_windows(sk);
        return d;
    }
    void append(const SketchSet &d, uint32_t first, uint32_t last)   // genomes [first, last) of a download
    {
        if (out.wide()) out.hashes64.insert(out.hashes64.end(), d.hashes64.begin() + d.off[first], d.hashes64.begin() + d.off[last]);
        else out.hashes.insert(out.hashes.end(), d.hashes.begin() + d.off[first], d.hashes.begin() + d.off[last]);
        if (abund) out.counts.insert(out.counts.end(), d.counts.begin() + d.off[first], d.counts.begin() + d.off[last]);
        for (uint32_t i = first; i < last; i++) out.off.push_back(out.off.back() + (d.off[i + 1] - d.off[i]));
    }
    void slow_path(size_t file_idx, rk_sketches **sk)  // whole file through rk_sketch_batch_ex
    {
        vector<uint8_t> seq, qual;
        vector<uint64_t> rec_off, genome_rec{0};
        if (!RecordReader::read_file(files[file_idx], seq, rec_off, fq.fastq ? &qual : nullptr))
            die("cannot open the genome file: %s", files[file_idx].c_str());
        if (rec_off.empty()) rec_off.push_back(0);
        genome_rec.push_back(rec_off.size() - 1);
        gpu.check((abund ? rk_sketch_batch_counts : rk_sketch_batch_ex)(gpu.ctx, flt, seq.data(), fq.fastq ? qual.data() : nullptr, fq.least_qual, min_count(),
                                                                        rec_off.data(), rec_off.size() - 1, genome_rec.data(), 1, sk),
                  abund ? "rk_sketch_batch_counts" : "rk_sketch_batch_ex");
    }
    // rare: the genomes of a batch whose slots overflowed take the slow path, spliced in in list order
    void append_spliced(const Batch &bt, rk_sketches *sk)
    {
        const uint32_t nb = (uint32_t)(bt.last - bt.first);
        const SketchSet d = download(sk, nb);
        for (uint32_t i = 0; i < nb; i++) {
            if (!bt.slots[i].overflow) { append(d, i, i + 1); continue; }
            rk_sketches *one = nullptr;
            slow_path(bt.first + i, &one);
            append(download(one, 1), 0, 1);
            rk_sketches_free(one);
        }
    }

    // ---- one big file, streamed.  What the readers of sketch_input.hpp need of the GPU: a ring of page-locked buffers, one upload
    // and one synchronisation per piece, a device buffer that is copied when it grows, ONE sketch call over the complete buffer.
    struct GpuSink : InputSink {
        ListSketcher &job;
        rk_sketches **sk_out;
        void *d_buf = nullptr;
        double kernel_sec = 0;
        GpuSink(ListSketcher &j, rk_sketches **out) : job(j), sk_out(out) {}
        ~GpuSink() { rk_dev_free(d_buf); }
        uint8_t *ring_alloc(uint64_t bytes) override
        {
            uint8_t *p = nullptr;
            job.gpu.check(rk_pinned_alloc(job.gpu.ctx, bytes, (void **)&p), "rk_pinned_alloc");
            return p;
        }
        void ring_free(uint8_t *p) override { rk_pinned_free(p); }
        void grow(uint64_t cap, uint64_t used) override
        {
            void *d_new = nullptr;
            job.gpu.check(rk_dev_alloc(job.gpu.ctx, cap, &d_new), "rk_dev_alloc");
            if (used) {
                job.gpu.check(rk_dev_copy_async(job.gpu.ctx, d_new, d_buf, used, job.stream), "rk_dev_copy_async");
                job.gpu.check(rk_stream_sync(job.gpu.ctx, job.stream), "rk_stream_sync");
            }
            rk_dev_free(d_buf);
            d_buf = d_new;
        }
        void put(uint64_t off, const uint8_t *src, uint64_t bytes) override
        {
            job.gpu.check(rk_upload_async(job.gpu.ctx, (uint8_t *)d_buf + off, src, bytes, job.stream), "rk_upload_async");
            job.gpu.check(rk_stream_sync(job.gpu.ctx, job.stream), "rk_stream_sync");
        }
        void complete(uint64_t used) override
        {
            const double t = get_sec();
            const uint64_t gbeg = 0, gend = used;
            job.gpu.check(job.packed_call()(job.gpu.ctx, job.flt, (const uint8_t *)d_buf, used, &gbeg, &gend, 1, job.min_count(), job.stream, sk_out),
                          job.packed_name());
            kernel_sec = get_sec() - t;
        }
    };
    // A plain FASTA file is mapped and cut at line starts, anything else (gzip'ed, FASTQ) read sequentially.  Returns false --
    // nothing done -- for a file the streamed readers do not take ('\r' line ends, odd records).
    bool sketch_streamed(const string &path, rk_sketches **sk)
    {
        GpuSink sink(*this, sk);
        StreamStats st;
        const int kmer = 2 * shuf.k;
        const bool mapped = !fq.fastq && !ends_with(path, ".gz");
        const bool ok = mapped ? stream_mapped_fasta(path, kmer, threads, big_piece_bytes(), sink, st)
                               : stream_sequential(path, fq.fastq, fq.fastq ? fq.least_qual : 0, kmer, threads, big_piece_bytes(),
                                                   sequential_dev_cap(path), sink, st);
        if (timing && st.ring && mapped) {
            fprintf(stderr, "[timing] big file: %zu piece(s), %d x %.1f MB page-locked + %.1f MB device: %.3f s\n", st.pieces, st.ring,
                    st.slot_bytes / 1e6, st.dev_bytes / 1e6, st.alloc_sec);
            fprintf(stderr, "[timing] big file: parse + upload of %.1f MB (overlapped, %d thread(s)): %.3f s, sketch kernels: %.3f s\n",
                    st.text_bytes / 1e6, st.parsers, st.stream_sec, sink.kernel_sec);
        } else if (timing && st.ring)
            fprintf(stderr, "[timing] big file (sequential reader): %zu piece(s), %.1f MB of text, %.1f MB packed, read + parse + upload "
                    "(overlapped, %d parser thread(s)): %.3f s, sketch kernels: %.3f s\n", st.pieces, st.text_bytes / 1e6, st.used / 1e6, st.parsers,
                    st.stream_sec, sink.kernel_sec);
        return ok;
    }

    // ---- the parser stage of batch k (the calling thread and its pool)
    void parse_batch(size_t k)
    {
        const int slot = staging.acquire();   // the GPU thread has released this staging buffer
        Batch &bt = batches[k];
        if (bt.pageable && !getenv("RK_BIG_WHOLE")) {
            // a big file: the GPU thread streams it piece by piece (read / inflate, parse, upload and kernels overlap)
            bt.streamed = true;
            staging.publish(k, slot);
            return;
        }
        if (bt.pageable) {  // its own buffer; the previous oversized batch must be uploaded first: the other buffer is free too
            staging.release(staging.acquire());
            big_stage.resize(bt.bytes);
        }
        uint8_t *base = bt.pageable ? big_stage.data() : stage[slot];
        const size_t nb = bt.last - bt.first;
        const double t_parse = get_sec();
        std::atomic<size_t> next_file{0};
        std::atomic<int> failed{-1};
        const int nt = std::max(1, std::min<int>(threads, (int)nb));
        std::vector<std::thread> pool;
        for (int t = 0; t < nt; t++)
            pool.emplace_back([&]() {
                RawBuf buf;  // one allocation per thread, reused for all its files
                for (;;) {
                    const size_t i = next_file.fetch_add(1);
                    if (i >= nb) break;
                    Slot &sl = bt.slots[i];
                    size_t n = 0;
                    // a big plain file in a batch with idle parser threads: read and parse it in parallel
                    const int spare = std::max(1, threads / nt);
                    const bool big = spare > 1 && sl.cap >= (64u << 20) && !ends_with(files[bt.first + i], ".gz");
                    if (!(big ? RecordReader::slurp_parallel(files[bt.first + i], buf, n, spare)
                              : RecordReader::slurp(files[bt.first + i], buf, n))) { failed = (int)i; continue; }
                    RecordReader::Packed pk;
                    if (!(big && !fq.fastq &&
                          RecordReader::parse_packed_parallel(buf.data(), n, base + sl.off, sl.cap, spare, pk)))
                        pk = RecordReader::parse_packed(buf.data(), n, base + sl.off, sl.cap, fq.fastq ? fq.least_qual : 0);
                    sl.overflow = pk.overflow;
                    sl.len = pk.overflow ? 0 : pk.bytes;
                    // zero-fill up to the next multiple of 1024 (the kernel reads whole 1 KiB lines)
                    const uint64_t end = sl.len, pad_end = std::min<uint64_t>(sl.cap, (end + 1024) & ~1023ULL);
                    memset(base + sl.off + end, 0, pad_end - end);
                }
            });
        for (auto &th : pool) th.join();
        if (timing) fprintf(stderr, "[timing] batch %zu: read + parse of %zu file(s) on %d thread(s): %.3f s\n", k, nb, nt, get_sec() - t_parse);
        if (failed >= 0) die("cannot open the genome file: %s", files[bt.first + (size_t)failed].c_str());
        staging.publish(k, slot);
    }

    // ---- the GPU stage of batch k (the GPU thread)
    void gpu_batch(size_t k, int bi)
    {
        Batch &bt = batches[k];
        const uint32_t nb = (uint32_t)(bt.last - bt.first);
        rk_sketches *sk = nullptr;
        bool any_overflow = false;
        if (bt.streamed) {
            if (!sketch_streamed(files[bt.first], &sk)) slow_path(bt.first, &sk);   // the serial reader
        } else {
            vector<uint64_t> gbeg(nb), gend(nb);
            for (uint32_t i = 0; i < nb; i++) {
                gbeg[i] = bt.slots[i].off;
                gend[i] = bt.slots[i].off + (bt.slots[i].overflow ? 0 : bt.slots[i].len);
                any_overflow |= bt.slots[i].overflow;
            }
            const double t_gpu = get_sec();
            gpu.check(rk_upload_async(gpu.ctx, dev[bi], bt.pageable ? big_stage.data() : stage[bi], bt.bytes, stream), "rk_upload_async");
            gpu.check(packed_call()(gpu.ctx, flt, (const uint8_t *)dev[bi], bt.bytes, gbeg.data(), gend.data(), nb, min_count(), stream, &sk), packed_name());
            if (timing) fprintf(stderr, "[timing] batch %zu: upload + sketch of %.1f MB: %.3f s\n", k, bt.bytes / 1e6, get_sec() - t_gpu);
        }
        staging.release(bi);   // the call above synchronised the stream: the staging buffer can be refilled
        if (any_overflow) append_spliced(bt, sk);
        else append(download(sk, nb), 0, nb);
        rk_sketches_free(sk);
        cerr << "finshed sketching: " << bt.last << " genomes" << endl;
    }

    void run()
    {
        plan();
        alloc_buffers();
        std::thread gpu_thread([&]() {
            size_t k = 0;
            int slot = 0;
            while (staging.take(k, slot)) gpu_batch(k, slot);
        });
        for (size_t k = 0; k < batches.size(); k++) parse_batch(k);
        staging.producer_done();
        gpu_thread.join();
        free_buffers();
    }
};

static void sketch_list(Gpu &gpu, const string &list, const Shuf &shuf, int threads, SketchSet &out, const string &out_path_in,
                        const FastqOpts &fq = FastqOpts(), bool abund = false)
{
    const double t0 = get_sec();
    rk_params P;
    if (rk_params_init(shuf.k, shuf.subk, shuf.drlevel, &P))
        die("the half_subk - drlevel should at least 3 (half_subk=%d drlevel=%d), half_k >= half_subk, half_subk < 8",
            shuf.subk, shuf.drlevel);  // src/common.cpp:37
    rk_filter *flt = nullptr;
    gpu.check(rk_filter_create(gpu.ctx, &P, shuf.table.data(), &flt), "rk_filter_create");
    if (getenv("RK_TIMING")) fprintf(stderr, "[timing] rk_filter_create: %.3f s\n", get_sec() - t0);

    const vector<string> files = read_list(list);
    cerr << "the total fileNumber is: " << files.size() << endl;
    out = SketchSet();
    out.info.half_k = shuf.k;
    out.info.half_subk = shuf.subk;
    out.info.drlevel = shuf.drlevel;
    out.names = files;
    out.off.assign(1, 0);

    ListSketcher job{gpu, flt, files, shuf, threads, fq, out, abund};
    job.run();
    rk_filter_free(flt);

    string out_path = out_path_in;
    if (!is_sketch_file(out_path)) out_path += ".sketch";  // src/sketch.cpp:570-572
    string err;
    if (!save_sketches(out_path, out, err)) die("%s", err.c_str());
    cerr << "save the sketches into: " << out_path << endl;
    if (abund) {   // the occurrence counts, next to the .sketch (which stays the reference's format)
        if (!save_abund(abund_path(out_path), out, err)) die("%s", err.c_str());
        cerr << "save the occurrence counts into: " << abund_path(out_path) << endl;
    }
    cerr << "===================time of sketching " << files.size() << " genomes (" << job.total_windows
         << " k-mers) is: " << get_sec() - t0 << endl;
}

static rk_sketches *upload(Gpu &gpu, const SketchSet &s)
{
    rk_sketches *sk = nullptr;
    if (s.wide())
        gpu.check(rk_sketches_from_host64(gpu.ctx, s.hashes64.data(), s.off.data(), (uint32_t)s.size(), &sk),
                  "rk_sketches_from_host64");
    else
        gpu.check(rk_sketches_from_host(gpu.ctx, s.hashes.data(), s.off.data(), (uint32_t)s.size(), &sk),
                  "rk_sketches_from_host");
    return sk;
}

// the sketches of s with their counts (s.counts, read_abund) on the device: a counted sketch ascends, so every sketch goes up with its
// (hash, count) pairs in ascending hash order, whatever order the file had
static rk_sketches *upload_counted(Gpu &gpu, const SketchSet &s)
{
    const uint64_t total = s.total();
    vector<uint32_t> counts(total);
    vector<uint64_t> hashes(total), order;
    for (size_t g = 0; g < s.size(); g++) {
        order.resize(s.off[g + 1] - s.off[g]);
        for (uint64_t i = 0; i < order.size(); i++) order[i] = s.off[g] + i;
        auto hash_at = [&](uint64_t i) { return s.wide() ? s.hashes64[i] : (uint64_t)s.hashes[i]; };
        std::sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) { return hash_at(x) < hash_at(y); });
        for (uint64_t i = 0; i < order.size(); i++) {
            hashes[s.off[g] + i] = hash_at(order[i]);
            counts[s.off[g] + i] = s.counts[order[i]];
        }
    }
    vector<uint32_t> narrow;
    if (!s.wide()) narrow.assign(hashes.begin(), hashes.end());
    rk_sketches *sk = nullptr;
    gpu.check(rk_sketches_from_host_counts(gpu.ctx, s.wide() ? (const void *)hashes.data() : (const void *)narrow.data(), s.wide() ? 1 : 0, counts.data(), s.off.data(),
                                           (uint32_t)s.size(), &sk), "rk_sketches_from_host_counts");
    return sk;
}

// -q of `screen --abund` / `mask --abund` is a .sketch file (checked before anything is read or sketched), with its side-car, or a message
static void need_sketch_queries(const Args &a, const char *who)
{
    if (a.has("abund") && !is_sketch_file(a.str("q", "")))
        die("%s --abund needs -q x.sketch with its x.sketch.abund (sketch --abund writes both), not a list of sequence files", who);
}
static void need_counted_queries(const char *who, const string &qry_path, SketchSet &qry)
{
    string err;
    if (!read_abund(abund_path(qry_path), qry, err)) die("%s --abund needs the occurrence counts of the queries, %s.abund (sketch --abund writes it): %s", who, qry_path.c_str(), err.c_str());
}

// builds the index on the GPU and, when asked, writes <sketch>.dict/.index (transSketches,
// src/sketch.cpp:894-1021)
static rk_index *build_index(Gpu &gpu, const SketchSet &s, const string &sketch_path, bool write_files)
{
    const double t0 = get_sec();
    const int bits = 4 * (s.info.half_k - s.info.drlevel);
    rk_sketches *sk = upload(gpu, s);
    rk_index *idx = nullptr;
    gpu.check(rk_index_build(gpu.ctx, sk, bits, &idx), "rk_index_build");
    rk_sketches_free(sk);
    if (write_files) {
        string err;
        vector<uint32_t> postings(rk_index_total(idx));
        if (s.wide()) {  // sparse layout, src/sketch.cpp:942-963
            vector<uint64_t> hashes(rk_index_distinct(idx));
            vector<uint32_t> counts(rk_index_distinct(idx));
            gpu.check(rk_index_export64(idx, postings.data(), hashes.data(), counts.data()), "rk_index_export64");
            if (!write_index64(sketch_path + ".dict", sketch_path + ".index", postings, hashes, counts, err)) die("%s", err.c_str());
        } else if (getenv("RK_INDEX_WRITE_LISTS")) {   // dense layout from the sparse form, scattered on the host (measured slower:
                                                          // 0.52-0.62 s against 0.28 s for 1,000 genomes at 28 hash bits)
            vector<uint32_t> hashes(rk_index_distinct(idx)), counts(rk_index_distinct(idx));
            gpu.check(rk_index_export_lists(idx, postings.data(), hashes.data(), counts.data()), "rk_index_export_lists");
            if (!write_index_lists(sketch_path + ".dict", sketch_path + ".index", postings.data(), postings.size(), hashes.data(),
                                   counts.data(), hashes.size(), (uint64_t)1 << bits, err,
                                   (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()))))
                die("%s", err.c_str());
        } else {         // dense layout, src/sketch.cpp:991-1011
            RawBuf counts;  // 4 * 2^bits bytes, every one of them written by the export: no zero-fill
            counts.resize((size_t)4 << bits);
            gpu.check(rk_index_export(idx, postings.data(), (uint32_t *)counts.data()), "rk_index_export");
            if (!write_index(sketch_path + ".dict", sketch_path + ".index", postings.data(), postings.size(),
                             (const uint32_t *)counts.data(), (uint64_t)1 << bits, err,
                             (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()))))
                die("%s", err.c_str());
        }
    }
    cerr << "===============the time of transSketches is: " << get_sec() - t0 << endl;
    return idx;
}

// ---- distance text (src/dist.cpp:233,256,263-336 / :642,690,696-770) --------------------------------------------
// The reference's worker threads each append their rows to a sub-file `<out>.dir/<out>.<tid>` and note
// "rowName\tsubFile" in `<out>.index.<tid>`; afterwards the sub-files are concatenated into <out> behind the header
// line when they total at most 4 GiB, otherwise they stay and the notes become `<out>.index` (:276-336).  Here a
// worker is a (GPU, formatter thread) pair: every GPU's hits (sorted by row) are cut at row boundaries into pieces,
// each piece is formatted once by one thread, and the pieces are either written into <out> with concurrent pwrites
// or kept as the sub-files.  Every row is listed exactly once in the index, hits or not, like the reference's.
struct HitPart {              // what one GPU computed
    const rk_hit *hits = nullptr;
    uint64_t n = 0;
    vector<uint32_t> rows;    // the rows it owns, ascending
};

static uint64_t max_merge_bytes()
{
    const char *v = getenv("RK_DIST_MAX_MERGE_BYTES");  // tests force the split on small outputs
    return v && atoll(v) > 0 ? (uint64_t)atoll(v) : 1ULL << 32;
}

static void write_hits(const string &out, const vector<HitPart> &parts, bool alldist, const vector<string> &rows,
                       const vector<string> &cols, int threads = 1)
{
    const double t0 = get_sec();
    const uint64_t max_size = max_merge_bytes();
    auto line = [&](const rk_hit &h, char *buf, size_t cap) {
        const string &a = alldist ? cols[h.col] : rows[h.row];
        const string &b = alldist ? rows[h.row] : cols[h.col];
        if (a.size() + b.size() + 128 > cap) die("genome name too long");
        return rk_format_hit(buf, cap, a.c_str(), b.c_str(), &h);
    };
    struct Piece {
        const rk_hit *hits;
        uint64_t n;
        const uint32_t *row_begin, *row_end;  // rows listed under this piece in the index
        string text;
    };
    vector<Piece> pieces;
    const int per_part = std::max(1, std::max(1, threads) / (int)std::max<size_t>(1, parts.size()));
    for (const HitPart &pt : parts) {
        // cut the part into up to per_part pieces of ~equal hit counts at row boundaries
        // (pieces of ~4,096 hits: the 45,000 lines of a 10,000-genome alldist were ONE piece, formatted by one thread in 10 ms)
        uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)per_part * 4, (pt.n + 4095) / 4096));
        if (max_size != (1ULL << 32)) want = (uint64_t)per_part;  // sub-file layout under test: one piece per worker
        uint64_t i0 = 0;
        size_t r0 = 0;
        for (uint64_t p = 0; p < want; p++) {
            uint64_t i1 = p + 1 == want ? pt.n : std::max(i0, pt.n / want * (p + 1));
            while (i1 < pt.n && i1 > 0 && pt.hits[i1].row == pt.hits[i1 - 1].row) i1++;  // whole rows
            size_t r1 = pt.rows.size();
            if (p + 1 < want && i1 < pt.n) r1 = std::lower_bound(pt.rows.begin(), pt.rows.end(), pt.hits[i1].row) - pt.rows.begin();
            if (p + 1 == want) i1 = pt.n;
            pieces.push_back(Piece{pt.hits + i0, i1 - i0, pt.rows.data() + r0, pt.rows.data() + r1, string()});
            i0 = i1;
            r0 = r1;
        }
    }
    const uint64_t n_pieces = pieces.size();
    {
        std::atomic<uint64_t> next{0};
        auto work = [&]() {
            vector<char> lb(1 << 16);
            for (;;) {
                const uint64_t p = next.fetch_add(1);
                if (p >= n_pieces) break;
                string &t = pieces[p].text;
                t.reserve((size_t)pieces[p].n * 72);
                for (uint64_t i = 0; i < pieces[p].n; i++) t.append(lb.data(), (size_t)line(pieces[p].hits[i], lb.data(), lb.size()));
            }
        };
        vector<std::thread> pool;
        for (int t = 1; t < std::max(1, threads) && (uint64_t)t < n_pieces; t++) pool.emplace_back(work);
        work();
        for (auto &th : pool) th.join();
    }
    uint64_t total = 0;
    for (const Piece &pc : pieces) total += pc.text.size();
    std::atomic<int> failed{0};
    if (total <= max_size) {  // isMerge, src/dist.cpp:286-310
        cerr << "-----save the output distance file: " << out << endl;
        const char *head = " genome0\tgenome1\tcommon|size0|size1\tjaccard\tmashD\n";
        const int fd = open(out.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) die("cannot write %s", out.c_str());
        bool good = pwrite(fd, head, strlen(head), 0) == (ssize_t)strlen(head);
        vector<uint64_t> at(n_pieces);
        uint64_t pos = strlen(head);
        for (uint64_t p = 0; p < n_pieces; p++) { at[p] = pos; pos += pieces[p].text.size(); }
        std::atomic<uint64_t> next{0};
        auto put = [&]() {
            for (;;) {
                const uint64_t p = next.fetch_add(1);
                if (p >= n_pieces) break;
                const string &t = pieces[p].text;
                uint64_t done = 0;
                while (done < t.size()) {
                    const ssize_t r = pwrite(fd, t.data() + done, t.size() - done, (off_t)(at[p] + done));
                    if (r <= 0) { failed = 1; break; }
                    done += (uint64_t)r;
                }
            }
        };
        vector<std::thread> pool;
        for (int t = 1; t < std::min(8, std::max(1, threads)) && (uint64_t)t < n_pieces; t++) pool.emplace_back(put);
        put();
        for (auto &th : pool) th.join();
        if (close(fd) || failed || !good) die("write error on %s", out.c_str());
    } else {  // src/dist.cpp:311-335: the sub-files stay, <out>.index maps every row to its sub-file
        const string dir = out + ".dir";
        if (mkdir(dir.c_str(), 0777) && errno != EEXIST) die("cannot create %s", dir.c_str());
        cerr << "-----the output distance file is too big to merge into one single file, saving the result into directory: "
             << dir << endl;
        const string index_path = out + ".index";
        cerr << "-----save the index between genomes and distance sub-files into: " << index_path << endl;
        auto sub_name = [&](uint64_t p) { return dir + '/' + out + '.' + std::to_string(p); };  // :154 / :543
        std::atomic<uint64_t> next{0};
        auto put = [&]() {
            for (;;) {
                const uint64_t p = next.fetch_add(1);
                if (p >= n_pieces) break;
                FILE *fp = fopen(sub_name(p).c_str(), "w");
                if (!fp || fwrite(pieces[p].text.data(), 1, pieces[p].text.size(), fp) != pieces[p].text.size()) failed = 1;
                if (fp && fclose(fp)) failed = 1;
            }
        };
        vector<std::thread> pool;
        for (int t = 1; t < std::min(8, std::max(1, threads)) && (uint64_t)t < n_pieces; t++) pool.emplace_back(put);
        put();
        for (auto &th : pool) th.join();
        FILE *fidx = fopen(index_path.c_str(), "w");
        if (!fidx) die("cannot write %s", index_path.c_str());
        fprintf(fidx, "genomeName\tdistFileName\n");
        for (uint64_t p = 0; p < n_pieces; p++) {
            const string name = sub_name(p);
            for (const uint32_t *r = pieces[p].row_begin; r != pieces[p].row_end; ++r) fprintf(fidx, "%s\t%s\n", rows[*r].c_str(), name.c_str());
        }
        if (fclose(fidx) || failed) die("write error under %s", dir.c_str());
    }
    cerr << "===================time of merge the subFiles into final files is: " << get_sec() - t0 << endl;
}

static void load_or_sketch(Gpu &gpu, const string &input, const Args &a, int threads, SketchSet &s,
                           string &sketch_path)
{
    string err;
    if (is_sketch_file(input)) {
        sketch_path = input;
        if (!read_sketches(input, s, err)) die("readSketches(), %s", err.c_str());
        return;
    }
    // list of FASTA files (src/subCommand.cpp:174-181): sketch into <list>.sketch
    const vector<string> files = read_list(input);
    if (files.empty()) die("cannot open the inputFile or empty list: %s", input.c_str());
    FastqOpts fq;
    fq.fastq = list_is_fastq(files);
    fq.least_qual = a.num("Q", 0);
    fq.least_num = a.num("n", 1);
    Shuf shuf;
    const string shuf_file = a.str("L", "shuf_file/L3K10.shuf");
    cerr << "---read the shuffle file: " << shuf_file << endl;
    if (!read_shuf(shuf_file, shuf, err)) die("read_shuffle_dim(), %s", err.c_str());
    sketch_path = input + ".sketch";
    sketch_list(gpu, input, shuf, threads, s, sketch_path, fq);
}

static int cmd_shuffle(const Args &a)
{
    const string out = a.str("o", "result.out");
    cerr << "-----generate the shuffle file: " << out << endl;
    string err;
    if (!write_shuf(out, a.num("k", 10), a.num("s", 6), a.num("l", 3), err)) die("write_shuffle_dim_file(), %s", err.c_str());
    return 0;
}

static int cmd_sketch(const Args &a)
{
    if (!a.has("i") || !a.has("o")) die("sketch needs -i and -o");
    const string in = a.str("i", ""), out = a.str("o", "");
    const bool is_query = a.has("q");
    const int threads = a.num("t", (int)std::thread::hardware_concurrency());
    if (a.has("abund") && is_sketch_file(in)) die("sketch --abund needs sequence files: a .sketch file holds no occurrence counts");
    Gpu gpu(a.num("device", 0));
    string err;
    if (is_sketch_file(in)) {  // src/main.cpp:189-214: copy, and (re)build the index unless -q
        SketchSet s;
        if (!read_sketches(in, s, err)) die("readSketches(), %s", err.c_str());
        if (!save_sketches(out, s, err)) die("%s", err.c_str());
        if (!is_query) rk_index_free(build_index(gpu, s, out, true));
        return 0;
    }
    Shuf shuf;
    const string shuf_file = a.str("L", "shuf_file/L3K10.shuf");
    cerr << "---read the shuffle file: " << shuf_file << endl;
    if (!read_shuf(shuf_file, shuf, err)) die("read_shuffle_dim(), %s", err.c_str());
    FastqOpts fq;
    fq.fastq = list_is_fastq(read_list(in));
    fq.least_qual = a.num("Q", 0);
    fq.least_num = a.num("n", 1);
    SketchSet s;
    string out_path = out;
    sketch_list(gpu, in, shuf, threads, s, out_path, fq, a.has("abund"));
    if (!is_sketch_file(out_path)) out_path += ".sketch";
    if (!is_query) rk_index_free(build_index(gpu, s, out_path, true));
    return 0;
}

// ---- several GPUs in one process (rows are independent: `#pragma omp parallel for` over rows, src/dist.cpp:174,560)
// One context and one host thread per GPU.  Every GPU builds its own copy of the index from the host's sketches
// (build_everywhere; RK_MULTI_BROADCAST=1: built once, replicated with rk_index_broadcast); alldist deals blocks of 32 rows round-robin,
// dist hands every GPU a contiguous block of queries; per-GPU hits go to the writer as they are (no reduction).
struct GpuSet {
    vector<std::unique_ptr<AsyncGpu>> gpus;
    GpuSet(int first_device, int n, bool same_device)
    {
        if (n < 1) die("--gpus must be at least 1");
        for (int g = 0; g < n; g++) gpus.emplace_back(new AsyncGpu(same_device ? first_device : first_device + g));
    }
    size_t size() const { return gpus.size(); }
    Gpu &operator[](size_t g) { return gpus[g]->get(); }
};

// f(g) for every GPU of a set: GPUs 1 .. G-1 on threads of their own, GPU 0 on the caller; back when all are through
template <class F> static void on_every_gpu(size_t G, F &&f)
{
    vector<std::thread> pool;
    for (size_t g = 1; g < G; g++) pool.emplace_back([&f, g] { f(g); });
    f(0);
    for (auto &th : pool) th.join();
}

static const int kRowBlock = 32;   // rows are dealt to the GPUs in blocks of 32: a multiple of the tile kernel's block, an even number for the row pairs

// The index on every GPU of the set.  Default: every GPU uploads the sketches over its own PCIe link and builds its own
// index, all at the same time (the build is deterministic: same internal genome order, same postings everywhere) -- 49 MB
// of sketches and 0.5 ms of build per GPU at 10,000 genomes, against a 147 MB blob pulled from the first GPU once IT is done.
// RK_MULTI_BROADCAST=1: build on the first GPU, replicate with rk_index_broadcast (peer copies over xGMI).
static void build_everywhere(GpuSet &set, const SketchSet &s, const string &path, bool write_files, vector<rk_index *> &idx)
{
    const size_t G = set.size();
    if (G > 1 && getenv("RK_MULTI_BROADCAST") && atoi(getenv("RK_MULTI_BROADCAST"))) {
        idx[0] = build_index(set[0], s, path, write_files);
        vector<rk_ctx *> peers;
        for (size_t g = 1; g < G; g++) peers.push_back(set[g].ctx);
        set[0].check(rk_index_broadcast(idx[0], peers.data(), (uint32_t)peers.size(), idx.data() + 1), "rk_index_broadcast");
        return;
    }
    on_every_gpu(G, [&](size_t g) { idx[g] = build_index(set[g], s, path, g == 0 && write_files); });
}

// The frame of the self-join subcommands (alldist, cluster, forest, greedy, knn, dbscan, mreach, medoid): the common arguments, the input (a .sketch file, or a
// genome list that is sketched first), the index on every GPU of the set (the sharded build where it applies, the whole index
// everywhere otherwise), the reference's phase lines around them and the way out.
struct SelfJoin {
    const Args &a;
    const double max_dist;
    const string out;
    const int metric, threads;
    std::unique_ptr<GpuSet> gpus;
    SketchSet s;
    vector<rk_index *> idx;   // one per GPU
    bool sharded = false;     // idx[g] is the join-only index of GPU g's rows
    double t1 = 0;            // start of the distance phase
    size_t G = 0, N = 0;      // GPUs, genomes

    // The common arguments and what every command refuses in them.  ordered: the command ranks pairs, so it refuses the dense report
    // (-D above 1.0) that alldist and cluster accept.  Nothing is opened or started here: the command's own refusals come next.
    SelfJoin(const Args &args, const char *cmd, bool ordered)
        : a(args), max_dist(a.real("D", 1.0)), out(a.str("o", "result.out")), metric(a.num("M", 0)),
          threads(a.num("t", (int)std::thread::hardware_concurrency()))
    {
        if (!a.has("i")) die("%s needs -i", cmd);
        if (max_dist < 0.0) die("command_%s(), maxDist must be > 0\nUse -D to set the maxDist", cmd);
        if (ordered && 1.0 < max_dist) die("command_%s(), maxDist must not exceed 1.0: pairs that share nothing carry no order", cmd);
    }
    // the GPUs first: their runtimes start on threads of their own while the .sketch file is read
    void prepare(int n_gpus, bool same_device)
    {
        gpus.reset(new GpuSet(a.num("device", 0), n_gpus, same_device));
        G = gpus->size();
        build();
        N = s.size();
    }
    void prepare() { prepare(a.num("gpus", 1), a.has("same-device")); }
    Gpu &gpu(size_t g) { return (*gpus)[g]; }
    // the options of GPU g's rows
    rk_dist_opts opts(size_t g) const
    {
        rk_dist_opts o{};
        o.triangle = 1;
        o.metric = metric;
        o.kmer_size = 2 * s.info.half_k;
        o.max_dist = max_dist;
        if (G > 1 && !sharded) {   // (a join-only index of the sharded flow holds this GPU's rows and nothing else)
            o.row_first = (uint32_t)g;
            o.row_step = (uint32_t)G;
            o.row_block = kRowBlock;
        }
        return o;
    }
    // the results are on the host: the stamp and the reference's phase line
    void phase_done(const char *what, const char *phase) const
    {
        stamp(what);
        cerr << "===================time of multiple threads distance computing and " << phase << " is: " << get_sec() - t1 << endl;
    }
    // The output is on disk and the process is about to end: handing 50 MB of sketches, the hit records and the index back block
    // by block costs 4-5 ms that buy nothing (the tool's last stamp).  Straight out, like the GPU subcommands' `leave` in main.
    [[noreturn]] static void leave()
    {
        stamp("text written");
        stamp("done");
        fflush(stdout);
        fflush(stderr);
        _exit(0);
    }

private:
    void build();
};

void SelfJoin::build()
{
    GpuSet &set = *gpus;
    const double t0 = get_sec();
    string sketch_path;
    if (is_sketch_file(a.str("i", ""))) {  // read while the runtime starts
        string err;
        sketch_path = a.str("i", "");
        if (!read_sketches(sketch_path, s, err)) die("readSketches(), %s", err.c_str());
    }
    Gpu &gpu = set[0];
    if (sketch_path.empty()) load_or_sketch(gpu, a.str("i", ""), a, threads, s, sketch_path);
    stamp("sketches read");
    // the .dict/.index pair is (re)written only if missing (src/subCommand.cpp:165-169); the
    // device index is always rebuilt from the sketches: faster than reading the 2^bits array
    const bool missing = !exist_file(sketch_path + ".index") || !exist_file(sketch_path + ".dict");
    idx.assign(G, nullptr);
    // Several GPUs (round 5): the all-vs-all shards twice -- every GPU builds the posting lists of ITS range of the hash space, the
    // tile records change hands once (GPU d pulls what belongs to its rows over its own links), every GPU sorts what arrived and
    // joins its rows.  No index is replicated.  Taken for a power-of-two number of GPUs when the .dict / .index pair exists (writing
    // them needs the whole index on one GPU) and the collection takes the bucket sort with tile records (set sketches, 2 and more
    // genomes); anything else -- and RK_MULTI_REPLICATE=1 -- builds the whole index on every GPU as before.
    // (a dense report -- -D above 1.0: every pair -- needs counter rows over slice records, which a join-only index has not)
    sharded = G > 1 && (G & (G - 1)) == 0 && !missing && !(1.0 < max_dist) && !(getenv("RK_MULTI_REPLICATE") && atoi(getenv("RK_MULTI_REPLICATE")));
    if (sharded) {
        const int bits = 4 * (s.info.half_k - s.info.drlevel);
        vector<rk_index *> part(G, nullptr);
        vector<int> rcs(G, 0);
        auto build_part = [&](size_t g) {
            rk_sketches *sk = upload(set[g], s);
            rcs[g] = rk_index_build_shard(set[g].ctx, sk, bits, (uint32_t)g, (uint32_t)G, &part[g]);
            rk_sketches_free(sk);
        };
        on_every_gpu(G, build_part);
        bool ok = true;
        for (size_t g = 0; g < G; g++) ok = ok && rcs[g] == 0;
        vector<void *> recv(G, nullptr);
        vector<uint64_t> n_recv(G, 0);
        if (ok) ok = rk_index_shard_exchange(part.data(), (uint32_t)G, recv.data(), n_recv.data()) == 0;
        if (ok) stamp("shards built, tile records exchanged");
        if (ok) {
            on_every_gpu(G, [&](size_t g) { rcs[g] = rk_index_join_shard(set[g].ctx, part[g], recv[g], n_recv[g], &idx[g]); });
            for (size_t g = 0; g < G; g++) ok = ok && rcs[g] == 0;
        }
        for (size_t g = 0; g < G; g++) {
            rk_dev_free(recv[g]);
            rk_index_free(part[g]);
            if (!ok && idx[g]) { rk_index_free(idx[g]); idx[g] = nullptr; }
        }
        if (!ok && getenv("RK_TIMING")) fprintf(stderr, "[timing] sharded build refused (%s): the whole index on every GPU\n", rk_last_error(set[0].ctx));
        sharded = ok;
    }
    if (!sharded) build_everywhere(set, s, sketch_path, missing, idx);
    stamp("index built");
    // (the reference's phase line, src/dist.cpp:132-135: there the phase loads .dict/.index, here it builds the index on the device)
    cerr << "===================time of read index and offset sketch file is: " << get_sec() - t0 << endl;
    t1 = get_sec();
    cerr << "=====total: " << s.size() << endl;
}

// ---- what the self-join subcommands share beyond the frame -----------------------------------------------------------------------
// GPU g's records folded into GPU 0's, g = 1 .. G-1: merge(g, &folded, &n_folded) is the library's fold of rec[0] and rec[g]
template <class Merge> static void fold_records(vector<rk_hit *> &rec, vector<uint64_t> &n_rec, const char *merge_name, Merge &&merge)
{
    for (size_t g = 1; g < rec.size(); g++) {
        rk_hit *folded = nullptr;
        uint64_t n_folded = 0;
        if (merge(g, &folded, &n_folded) != 0) die("%s failed", merge_name);
        rk_free_host(rec[0]);
        rk_free_host(rec[g]);
        rec[0] = folded;
        n_rec[0] = n_folded;
    }
}

// one line of alldist's format: the names as given, then the record
static void put_hit_line(FILE *fp, vector<char> &buf, const string &x, const string &y, const rk_hit &h)
{
    if (x.size() + y.size() + 128 > buf.size()) die("genome name too long");
    const int len = rk_format_hit(buf.data(), buf.size(), x.c_str(), y.c_str(), &h);
    if (len < 0) die("rk_format_hit failed");
    fwrite(buf.data(), 1, (size_t)len, fp);
}

// Members by cluster, clusters by representative: a counting sort over rep[] (rep[i] = the representative of i's cluster, i itself for
// a representative).  order: the genomes cluster by cluster, a representative first, then its members by ascending index (where the
// representative is the smallest member, as in cluster's labels, that is ascending throughout); number[r] and size[r]: of r's cluster.
struct ClusterOrder {
    vector<uint32_t> order, number, size;
    uint32_t n_clusters = 0;
    ClusterOrder(const vector<uint32_t> &rep, size_t N) : order(N), number(N, 0), size(N, 0)
    {
        vector<uint32_t> at(N + 1, 0);
        for (size_t i = 0; i < N; i++) size[rep[i]]++;
        for (size_t i = 0; i < N; i++) {
            at[i + 1] = at[i] + size[i];
            if (rep[i] == i) number[i] = n_clusters++;
        }
        for (size_t i = 0; i < N; i++)
            if (rep[i] == i) order[at[i]++] = (uint32_t)i;
        for (size_t i = 0; i < N; i++)
            if (rep[i] != i) order[at[rep[i]]++] = (uint32_t)i;
    }
};

static int cmd_alldist(const Args &a)
{
    SelfJoin j(a, "alldist", false);
    j.prepare();
    const size_t G = j.G;
    vector<rk_hit *> hits(G, nullptr);
    vector<uint64_t> n_hits(G, 0);
    on_every_gpu(G, [&](size_t g) {
        const rk_dist_opts o = j.opts(g);
        j.gpu(g).check(rk_dist_rows(j.gpu(g).ctx, j.idx[g], nullptr, &o, &hits[g], &n_hits[g], nullptr), "rk_dist_rows");
    });
    j.phase_done("distances on the host", "save the subFile");
    vector<HitPart> parts(G);
    for (size_t g = 0; g < G; g++) {
        parts[g].hits = hits[g];
        parts[g].n = n_hits[g];
        for (uint32_t r = 0; r < (uint32_t)j.N; r++)
            if (G == 1 || (r / kRowBlock) % G == g) parts[g].rows.push_back(r);
    }
    write_hits(j.out, parts, true, j.s.names, j.s.names, j.threads);
    j.leave();
}

// cluster: the single-linkage clusters of alldist's pairs (rk_cluster_rows on every GPU for its rows, folded with
// rk_cluster_merge), one line per genome: cluster number (clusters ordered by their representative, the member with the smallest
// index), cluster size, genome name; within a cluster the genomes by ascending index.
static int cmd_cluster(const Args &a)
{
    SelfJoin j(a, "cluster", false);
    j.prepare();
    const size_t G = j.G, N = j.N;
    vector<vector<uint32_t>> labels(G, vector<uint32_t>(N ? N : 1));
    vector<rk_cluster_stats> stats(G);
    on_every_gpu(G, [&](size_t g) {
        const rk_dist_opts o = j.opts(g);
        j.gpu(g).check(rk_cluster_rows(j.gpu(g).ctx, j.idx[g], &o, labels[g].data(), &stats[g]), "rk_cluster_rows");
    });
    for (size_t g = 1; g < G; g++)
        if (rk_cluster_merge(labels[0].data(), labels[g].data(), (uint32_t)N, labels[0].data()) != 0) die("rk_cluster_merge failed");
    j.phase_done("clusters on the host", "clustering");
    const vector<uint32_t> &lab = labels[0];   // (label[i] <= i, a representative labels itself)
    const ClusterOrder c(lab, N);
    FILE *fp = fopen(j.out.c_str(), "w");
    if (!fp) die("cannot write %s", j.out.c_str());
    for (size_t k = 0; k < N; k++) {
        const uint32_t i = c.order[k], rep = lab[i];
        fprintf(fp, "%u\t%u\t%s\n", c.number[rep], c.size[rep], j.s.names[i].c_str());
    }
    fclose(fp);
    if (getenv("RK_TIMING")) {
        unsigned long long edges = 0, border = 0;
        for (size_t g = 0; g < G; g++) { edges += stats[g].edges; border += stats[g].borderline; }
        fprintf(stderr, "[timing] %u clusters of %zu genomes from %llu hit records (%llu borderline)\n", c.n_clusters, N, edges, border);
    }
    j.leave();
}

// forest: the minimum spanning forest of alldist's pairs -- the single-linkage dendrogram up to -D (rk_forest_rows on every GPU for its
// rows, folded with rk_forest_merge), one alldist line per edge in forest order: nearest pair first, ties by exact ratio, then by
// the genomes' indices.
static int cmd_forest(const Args &a)
{
    SelfJoin j(a, "forest", true);
    j.prepare();
    const size_t G = j.G, N = j.N;
    vector<rk_hit *> edges(G, nullptr);
    vector<uint64_t> n_edges(G, 0);
    vector<rk_forest_stats> stats(G);
    on_every_gpu(G, [&](size_t g) {
        const rk_dist_opts o = j.opts(g);
        j.gpu(g).check(rk_forest_rows(j.gpu(g).ctx, j.idx[g], &o, &edges[g], &n_edges[g], &stats[g]), "rk_forest_rows");
    });
    fold_records(edges, n_edges, "rk_forest_merge", [&](size_t g, rk_hit **folded, uint64_t *n_folded) {
        return rk_forest_merge(edges[0], n_edges[0], edges[g], n_edges[g], (uint32_t)N, j.metric, folded, n_folded);
    });
    j.phase_done("forest on the host", "spanning forest");
    FILE *fp = fopen(j.out.c_str(), "w");
    if (!fp) die("cannot write %s", j.out.c_str());
    vector<char> buf(1 << 16);
    for (uint64_t k = 0; k < n_edges[0]; k++) {
        const rk_hit &h = edges[0][k];
        put_hit_line(fp, buf, j.s.names[h.col], j.s.names[h.row], h);   // (the order of an alldist line, src/dist.cpp:233)
    }
    fclose(fp);
    if (getenv("RK_TIMING")) {
        unsigned long long hits = 0, border = 0, rounds = 0;
        for (size_t g = 0; g < G; g++) { hits += stats[g].edges; border += stats[g].borderline; rounds = std::max<unsigned long long>(rounds, stats[g].rounds); }
        fprintf(stderr, "[timing] %llu forest edges over %zu genomes from %llu hit records (%llu borderline), %llu rounds\n",
                (unsigned long long)n_edges[0], N, hits, border, rounds);
    }
    j.leave();
}

// greedy: greedy incremental clustering of alldist's pairs (rk_greedy_rows; the rule of CD-HIT and clust-greedy: larger sketch first, a
// genome is a representative unless an earlier representative lies within -D, else it joins the nearest such), one line per genome:
// cluster number (clusters ordered by their representative's index), cluster size, genome name, representative's name, dist to it;
// within a cluster the representative first, then the members by ascending index.  --reps: the representatives' names alone.
static int cmd_greedy(const Args &a)
{
    SelfJoin j(a, "greedy", true);
    if (a.num("gpus", 1) > 1) die("command_greedy(), greedy runs on one GPU: the rule does not compose from the shards of several (--gpus 1)");
    j.prepare(1, false);
    const size_t N = j.N;
    vector<uint32_t> rep(N ? N : 1);
    rk_hit *links = nullptr;
    uint64_t n_links = 0;
    rk_greedy_stats stats{};
    const rk_dist_opts o = j.opts(0);
    j.gpu(0).check(rk_greedy_rows(j.gpu(0).ctx, j.idx[0], &o, nullptr, rep.data(), &links, &n_links, &stats), "rk_greedy_rows");
    j.phase_done("representatives on the host", "greedy clustering");
    const ClusterOrder c(rep, N);
    vector<double> dist(N, 0.0);
    for (size_t i = 0, k = 0; i < N; i++)
        if (rep[i] != i) dist[i] = links[k++].dist;   // (the links come by member index)
    FILE *fp = fopen(j.out.c_str(), "w");
    if (!fp) die("cannot write %s", j.out.c_str());
    for (size_t k = 0; k < N; k++) {
        const uint32_t i = c.order[k], r = rep[i];
        fprintf(fp, "%u\t%u\t%s\t%s\t%f\n", c.number[r], c.size[r], j.s.names[i].c_str(), j.s.names[r].c_str(), dist[i]);
    }
    fclose(fp);
    if (a.has("reps")) {
        FILE *rp = fopen(a.str("reps", "").c_str(), "w");
        if (!rp) die("cannot write %s", a.str("reps", "").c_str());
        for (size_t i = 0; i < N; i++)
            if (rep[i] == i) fprintf(rp, "%s\n", j.s.names[i].c_str());
        fclose(rp);
    }
    if (getenv("RK_TIMING"))
        fprintf(stderr, "[timing] %u representatives of %zu genomes from %llu hit records (%llu borderline), %u rounds\n", c.n_clusters, N,
                (unsigned long long)stats.edges, (unsigned long long)stats.borderline, stats.rounds);
    j.leave();
}

// knn: the k nearest neighbours of every genome among alldist's pairs -- the kNN graph within -D (rk_knn_rows on every GPU for its rows,
// folded with rk_knn_merge), one alldist-format line per (genome, neighbour): genomes by ascending index, nearest neighbour first, ties
// by exact ratio, then by the neighbour's index.  The genome's name comes first, the neighbour's second, and common|size|size follows
// that orientation.
static int cmd_knn(const Args &a)
{
    SelfJoin j(a, "knn", true);
    if (!a.has("N") || a.num("N", 0) < 1) die("command_knn(), maxNeighbor must be >= 1\nUse -N to set the maxNeighbor");
    const uint32_t k = (uint32_t)a.num("N", 1);
    j.prepare();
    const size_t G = j.G, N = j.N;
    vector<vector<uint64_t>> off(G, vector<uint64_t>(N + 1, 0));
    vector<rk_hit *> nbrs(G, nullptr);
    vector<uint64_t> n_nbrs(G, 0);
    vector<rk_knn_stats> stats(G);
    on_every_gpu(G, [&](size_t g) {
        const rk_dist_opts o = j.opts(g);
        j.gpu(g).check(rk_knn_rows(j.gpu(g).ctx, j.idx[g], &o, k, off[g].data(), &nbrs[g], &n_nbrs[g], &stats[g]), "rk_knn_rows");
    });
    fold_records(nbrs, n_nbrs, "rk_knn_merge", [&](size_t g, rk_hit **folded, uint64_t *n_folded) {
        return rk_knn_merge(off[0].data(), nbrs[0], off[g].data(), nbrs[g], (uint32_t)N, k, j.metric, off[0].data(), folded, n_folded);
    });
    j.phase_done("neighbours on the host", "neighbour selection");
    FILE *fp = fopen(j.out.c_str(), "w");
    if (!fp) die("cannot write %s", j.out.c_str());
    vector<char> buf(1 << 16);
    for (size_t i = 0; i < N; i++)
        for (uint64_t at = off[0][i]; at < off[0][i + 1]; at++) {
            rk_hit h = nbrs[0][at];
            const uint32_t other = h.row == i ? h.col : h.row;
            if (h.col == i) std::swap(h.size0, h.size1);   // the genome's size first
            put_hit_line(fp, buf, j.s.names[i], j.s.names[other], h);
        }
    fclose(fp);
    if (getenv("RK_TIMING")) {
        unsigned long long hits = 0, border = 0, most = 0, path = 0;
        for (size_t g = 0; g < G; g++) {
            hits += stats[g].edges;
            border += stats[g].borderline;
            most = std::max<unsigned long long>(most, stats[g].max_degree);
            path = std::max<unsigned long long>(path, stats[g].path);
        }
        fprintf(stderr, "[timing] %llu neighbour records (k = %u) over %zu genomes from %llu hit records (%llu borderline), largest degree %llu, path %llu\n",
                (unsigned long long)n_nbrs[0], k, N, hits, border, most, path);
    }
    j.leave();
}

// dbscan: density-based clusters of alldist's pairs (rk_dbscan_rows; a genome with -m genomes, itself included, within -D is core, the
// clusters are the components of the core genomes, a non-core genome next to a core one is a border genome of its nearest core
// neighbour's cluster, the rest is noise), one line per genome: cluster number (from 1, clusters ordered by their label, the smallest
// core index), cluster size, kind, genome name, degree, the name of the core neighbour a border genome came in through (else -);
// within a cluster the core genomes by ascending index, then the border genomes by ascending index; the noise last, as cluster 0 of
// size 0.
static int cmd_dbscan(const Args &a)
{
    SelfJoin j(a, "dbscan", true);
    if (a.num("gpus", 1) > 1) die("command_dbscan(), dbscan runs on one GPU: the core test does not compose from the shards of several (--gpus 1)");
    if (!a.has("m") || a.num("m", 0) < 1) die("command_dbscan(), minPts must be >= 1\nUse -m to set the minPts (it counts the genome itself)");
    const uint32_t min_pts = (uint32_t)a.num("m", 1);
    j.prepare(1, false);
    const size_t N = j.N;
    vector<uint32_t> label(N ? N : 1), via(N ? N : 1), degree(N ? N : 1);
    vector<uint8_t> kind(N ? N : 1);
    rk_dbscan_stats stats{};
    const rk_dist_opts o = j.opts(0);
    j.gpu(0).check(rk_dbscan_rows(j.gpu(0).ctx, j.idx[0], &o, min_pts, label.data(), kind.data(), via.data(), degree.data(), &stats), "rk_dbscan_rows");
    j.phase_done("density clusters on the host", "density clustering");
    // a counting sort by (label, kind descending): number[l] and size[l] of the cluster whose label is l
    vector<uint32_t> number(N, 0), size(N, 0), order(N);
    vector<size_t> at(N + 1, 0);
    size_t placed = 0;
    uint32_t n_clusters = 0;
    for (size_t i = 0; i < N; i++)
        if (kind[i]) size[label[i]]++;
    for (size_t l = 0; l < N; l++) {
        at[l] = placed;
        placed += size[l];
        if (size[l]) number[l] = ++n_clusters;
    }
    for (uint8_t k : {(uint8_t)2, (uint8_t)1, (uint8_t)0})
        for (size_t i = 0; i < N; i++)
            if (kind[i] == k) order[k ? at[label[i]]++ : placed++] = (uint32_t)i;
    static const char *const kind_name[3] = {"noise", "border", "core"};
    FILE *fp = fopen(j.out.c_str(), "w");
    if (!fp) die("cannot write %s", j.out.c_str());
    for (size_t k = 0; k < N; k++) {
        const uint32_t i = order[k];
        const uint32_t l = kind[i] ? label[i] : 0;
        fprintf(fp, "%u\t%u\t%s\t%s\t%u\t%s\n", kind[i] ? number[l] : 0u, kind[i] ? size[l] : 0u, kind_name[kind[i]], j.s.names[i].c_str(), degree[i],
                kind[i] == 1 ? j.s.names[via[i]].c_str() : "-");
    }
    fclose(fp);
    if (getenv("RK_TIMING"))
        fprintf(stderr, "[timing] %u density clusters (minPts = %u) of %zu genomes: %u core, %u border, %u noise, from %llu hit records (%llu borderline)\n",
                stats.n_clusters, min_pts, N, stats.n_core, stats.n_border, stats.n_noise, (unsigned long long)stats.edges, (unsigned long long)stats.borderline);
    j.leave();
}

// mreach: the minimum spanning forest of alldist's pairs under mutual-reachability distance -- the HDBSCAN* hierarchy up to -D
// (rk_mreach_rows; the core distance of a genome is the distance of its (minPts - 1)-th nearest pair within -D, the weight of a pair the
// largest of its own distance and its two genomes' core distances), one forest line per edge in forest order -- lightest first, ties by
// exact ratio, then by the genomes' indices -- with the mutual-reachability distance as a last column.  --core: one line per genome,
// name, core distance (- when the genome has fewer than minPts - 1 pairs), the name of the neighbour that sets it (- when none).
// --cut t --labels FILE: the forest cut at t (rk_mreach_cut) in the layout of cluster, clusters numbered from 1 by their smallest core
// genome, the genomes that are not core at t last, as cluster 0 of size 0.
static int cmd_mreach(const Args &a)
{
    SelfJoin j(a, "mreach", true);
    if (a.num("gpus", 1) > 1) die("command_mreach(), mreach runs on one GPU: the core distances do not compose from the shards of several (--gpus 1)");
    if (!a.has("m") || a.num("m", 0) < 1) die("command_mreach(), minPts must be >= 1\nUse -m to set the minPts (it counts the genome itself)");
    if (a.has("cut") != a.has("labels")) die("command_mreach(), --cut t and --labels FILE go together");
    const double cut = a.real("cut", 0.0);
    if (a.has("cut") && !(cut >= 0.0 && cut <= j.max_dist)) die("command_mreach(), --cut must lie between 0 and maxDist: the forest holds the hierarchy up to -D");
    const uint32_t min_pts = (uint32_t)a.num("m", 1);
    j.prepare(1, false);
    const size_t N = j.N;
    vector<double> core_dist(N ? N : 1);
    vector<uint32_t> core_nb(N ? N : 1);
    rk_hit *edges = nullptr;
    uint64_t n_edges = 0;
    rk_mreach_stats stats{};
    const rk_dist_opts o = j.opts(0);
    j.gpu(0).check(rk_mreach_rows(j.gpu(0).ctx, j.idx[0], &o, min_pts, core_dist.data(), core_nb.data(), &edges, &n_edges, &stats), "rk_mreach_rows");
    j.phase_done("mutual-reachability forest on the host", "mutual-reachability forest");
    FILE *fp = fopen(j.out.c_str(), "w");
    if (!fp) die("cannot write %s", j.out.c_str());
    vector<char> buf(1 << 16);
    for (uint64_t k = 0; k < n_edges; k++) {
        const rk_hit &h = edges[k];
        const string &x = j.s.names[h.col], &y = j.s.names[h.row];   // (the order of an alldist line, src/dist.cpp:233)
        if (x.size() + y.size() + 128 > buf.size()) die("genome name too long");
        const int len = rk_format_hit(buf.data(), buf.size(), x.c_str(), y.c_str(), &h);
        if (len < 1) die("rk_format_hit failed");
        fwrite(buf.data(), 1, (size_t)len - 1, fp);   // (without its newline)
        fprintf(fp, "\t%f\n", std::max(h.dist, std::max(core_dist[h.row], core_dist[h.col])));
    }
    fclose(fp);
    if (a.has("core")) {
        FILE *cp = fopen(a.str("core", "").c_str(), "w");
        if (!cp) die("cannot write %s", a.str("core", "").c_str());
        for (size_t i = 0; i < N; i++) {
            if (std::isinf(core_dist[i])) fprintf(cp, "%s\t-\t", j.s.names[i].c_str());
            else fprintf(cp, "%s\t%f\t", j.s.names[i].c_str(), core_dist[i]);
            fprintf(cp, "%s\n", core_nb[i] == RK_MREACH_NONE ? "-" : j.s.names[core_nb[i]].c_str());
        }
        fclose(cp);
    }
    if (a.has("cut")) {
        vector<uint32_t> label(N ? N : 1);
        if (rk_mreach_cut(edges, n_edges, core_dist.data(), (uint32_t)N, cut, label.data()) != 0) die("rk_mreach_cut failed");
        vector<uint32_t> number(N, 0), size(N, 0);
        uint32_t n_clusters = 0;
        for (size_t i = 0; i < N; i++)
            if (label[i] != RK_DBSCAN_NOISE) size[label[i]]++;
        for (size_t l = 0; l < N; l++)
            if (size[l]) number[l] = ++n_clusters;
        vector<vector<uint32_t>> members(N);   // (a label is its cluster's smallest genome: by label, then by index, is two ascending walks)
        for (size_t i = 0; i < N; i++)
            if (label[i] != RK_DBSCAN_NOISE) members[label[i]].push_back((uint32_t)i);
        FILE *lp = fopen(a.str("labels", "").c_str(), "w");
        if (!lp) die("cannot write %s", a.str("labels", "").c_str());
        for (size_t l = 0; l < N; l++)
            for (uint32_t i : members[l]) fprintf(lp, "%u\t%u\t%s\n", number[l], size[l], j.s.names[i].c_str());
        for (size_t i = 0; i < N; i++)
            if (label[i] == RK_DBSCAN_NOISE) fprintf(lp, "0\t0\t%s\n", j.s.names[i].c_str());
        fclose(lp);
    }
    if (getenv("RK_TIMING"))
        fprintf(stderr, "[timing] %llu mutual-reachability edges (minPts = %u) over %zu genomes, %u with a core distance, from %llu hit records (%llu borderline), %u rounds, path %u\n",
                (unsigned long long)n_edges, min_pts, N, stats.n_core, (unsigned long long)stats.edges, (unsigned long long)stats.borderline, stats.rounds, stats.path);
    j.leave();
}

// --labels FILE of medoid and assign: one line per genome of the clustered input in its order, an integer below their number N or - for
// an unlabelled genome (label[i] stays RK_MEDOID_NONE); dies in the name of `cmd` on anything else
static void read_labels(const string &path, size_t N, const char *cmd, vector<uint32_t> &label)
{
    std::ifstream in(path);
    if (!in) die("cannot read %s", path.c_str());
    string line;
    size_t seen = 0;
    while (std::getline(in, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (line.empty() && in.peek() == EOF) break;
        if (seen >= N) die("command_%s(), %s holds more than the %zu lines of the input", cmd, path.c_str(), N);
        if (line != "-") {
            char *end = nullptr;
            const unsigned long long v = strtoull(line.c_str(), &end, 10);
            if (line.empty() || *end || line[0] == '-' || line[0] == '+' || v >= N)
                die("command_%s(), line %zu of %s is neither an integer below %zu nor -", cmd, seen + 1, path.c_str(), N);
            label[seen] = (uint32_t)v;
        }
        seen++;
    }
    if (seen != N) die("command_%s(), %s holds %zu lines, the input %zu genomes", cmd, path.c_str(), seen, N);
}

// medoid: medoids and census of a clustering of alldist's pairs (rk_medoid_rows on every GPU for its rows, folded with rk_medoid_merge;
// rk_medoid_pick for the clusters).  The labels come from the same run -- --by cluster (the default; rk_cluster_rows, several GPUs), --by
// greedy (rk_greedy_rows: a cluster is a representative and its members), --by dbscan -m minPts (rk_dbscan_rows: noise is unlabelled) -- or
// from --labels FILE: one line per genome in input order, an integer below the number of genomes or - for an unlabelled genome.  One line
// per genome: cluster number (from 1, clusters by ascending label), cluster size, role (medoid or member), genome name, the pairs of the
// genome inside its cluster and leaving it, its mean similarity to its fellow members (central / 2^32 / (size - 1)), the name and
// distance of its nearest genome outside its cluster (- - when it has none within -D); within a cluster the medoid first, then the
// members by ascending index; the unlabelled genomes last, as cluster 0 of size 0 with role none.  --census: one line per cluster, its
// number, size, medoid, the pairs inside it, size (size - 1) / 2, its weakest inside pair (two names and the distance) and its
// nearest leaving pair.
static int cmd_medoid(const Args &a)
{
    SelfJoin j(a, "medoid", true);
    const string by = a.str("by", "cluster");
    if (a.has("by") && a.has("labels")) die("command_medoid(), --by and --labels exclude each other: the labels come from one place");
    if (by != "cluster" && by != "greedy" && by != "dbscan") die("command_medoid(), --by must be cluster, greedy or dbscan");
    const bool from_file = a.has("labels");
    if (!from_file && by != "cluster" && a.num("gpus", 1) > 1)
        die("command_medoid(), --by %s runs on one GPU: the rule does not compose from the shards of several (--gpus 1)", by.c_str());
    if (!from_file && by == "dbscan" && (!a.has("m") || a.num("m", 0) < 1))
        die("command_medoid(), minPts must be >= 1\nUse -m to set the minPts (it counts the genome itself)");
    j.prepare();
    const size_t G = j.G, N = j.N;
    vector<uint32_t> label(N ? N : 1, RK_MEDOID_NONE);
    if (from_file) {
        read_labels(a.str("labels", ""), N, "medoid", label);
    } else if (by == "cluster") {
        vector<vector<uint32_t>> labels(G, vector<uint32_t>(N ? N : 1));
        on_every_gpu(G, [&](size_t g) {
            const rk_dist_opts o = j.opts(g);
            j.gpu(g).check(rk_cluster_rows(j.gpu(g).ctx, j.idx[g], &o, labels[g].data(), nullptr), "rk_cluster_rows");
        });
        for (size_t g = 1; g < G; g++)
            if (rk_cluster_merge(labels[0].data(), labels[g].data(), (uint32_t)N, labels[0].data()) != 0) die("rk_cluster_merge failed");
        label = labels[0];
    } else if (by == "greedy") {
        rk_hit *links = nullptr;
        uint64_t n_links = 0;
        const rk_dist_opts o = j.opts(0);
        j.gpu(0).check(rk_greedy_rows(j.gpu(0).ctx, j.idx[0], &o, nullptr, label.data(), &links, &n_links, nullptr), "rk_greedy_rows");
        rk_free_host(links);
    } else {
        vector<uint8_t> kind(N ? N : 1);
        const rk_dist_opts o = j.opts(0);
        j.gpu(0).check(rk_dbscan_rows(j.gpu(0).ctx, j.idx[0], &o, (uint32_t)a.num("m", 1), label.data(), kind.data(), nullptr, nullptr, nullptr), "rk_dbscan_rows");
    }
    // the per-genome sums and records of every GPU's rows, folded into GPU 0's
    struct Part {
        vector<uint32_t> in_deg, out_deg;
        vector<uint64_t> central;
        vector<rk_hit> far_in, near_out;
        rk_medoid_genomes g;
        explicit Part(size_t n) : in_deg(n), out_deg(n), central(n), far_in(n), near_out(n), g{in_deg.data(), out_deg.data(), central.data(), far_in.data(), near_out.data()} {}
    };
    vector<std::unique_ptr<Part>> part(G);
    for (size_t g = 0; g < G; g++) part[g].reset(new Part(N ? N : 1));
    vector<rk_medoid_stats> stats(G);
    on_every_gpu(G, [&](size_t g) {
        const rk_dist_opts o = j.opts(g);
        j.gpu(g).check(rk_medoid_rows(j.gpu(g).ctx, j.idx[g], &o, label.data(), &part[g]->g, &stats[g]), "rk_medoid_rows");
    });
    for (size_t g = 1; g < G; g++)
        if (rk_medoid_merge(&part[0]->g, &part[g]->g, (uint32_t)N, j.metric, &part[0]->g) != 0) die("rk_medoid_merge failed");
    const Part &p = *part[0];
    rk_medoid_cluster *cl = nullptr;
    uint32_t n_cl = 0;
    if (rk_medoid_pick(label.data(), &p.g, (uint32_t)N, j.metric, &cl, &n_cl) != 0) die("rk_medoid_pick failed");
    j.phase_done("medoids on the host", "medoids and census");
    vector<vector<uint32_t>> members(n_cl);   // by cluster, ascending index
    {
        vector<uint32_t> at(N, 0);
        for (uint32_t k = 0; k < n_cl; k++) at[cl[k].label] = k;
        for (size_t i = 0; i < N; i++)
            if (label[i] != RK_MEDOID_NONE) members[at[label[i]]].push_back((uint32_t)i);
    }
    FILE *fp = fopen(j.out.c_str(), "w");
    if (!fp) die("cannot write %s", j.out.c_str());
    auto genome_line = [&](uint32_t number, uint32_t size, const char *role, uint32_t i) {
        const double mean = size > 1 ? (double)p.central[i] / 4294967296.0 / (double)(size - 1) : 0.0;
        fprintf(fp, "%u\t%u\t%s\t%s\t%u\t%u\t%.6f\t", number, size, role, j.s.names[i].c_str(), p.in_deg[i], p.out_deg[i], mean);
        const rk_hit &h = p.near_out[i];
        if (h.row == RK_MEDOID_NONE) fprintf(fp, "-\t-\n");
        else fprintf(fp, "%s\t%f\n", j.s.names[h.row == i ? h.col : h.row].c_str(), h.dist);
    };
    for (uint32_t k = 0; k < n_cl; k++) {
        genome_line(k + 1, cl[k].size, "medoid", cl[k].medoid);
        for (uint32_t i : members[k])
            if (i != cl[k].medoid) genome_line(k + 1, cl[k].size, "member", i);
    }
    for (size_t i = 0; i < N; i++)
        if (label[i] == RK_MEDOID_NONE) genome_line(0, 0, "none", (uint32_t)i);
    fclose(fp);
    if (a.has("census")) {
        FILE *cp = fopen(a.str("census", "").c_str(), "w");
        if (!cp) die("cannot write %s", a.str("census", "").c_str());
        auto pair = [&](const rk_hit &h) {
            if (h.row == RK_MEDOID_NONE) fprintf(cp, "\t-\t-\t-");
            else fprintf(cp, "\t%s\t%s\t%f", j.s.names[h.row].c_str(), j.s.names[h.col].c_str(), h.dist);
        };
        for (uint32_t k = 0; k < n_cl; k++) {
            fprintf(cp, "%u\t%u\t%s\t%llu\t%llu", k + 1, cl[k].size, j.s.names[cl[k].medoid].c_str(), (unsigned long long)cl[k].in_edges,
                    (unsigned long long)cl[k].size * (cl[k].size - 1) / 2);
            pair(cl[k].weakest_in);
            pair(cl[k].nearest_out);
            fprintf(cp, "\n");
        }
        fclose(cp);
    }
    if (getenv("RK_TIMING")) {
        unsigned long long hits = 0, border = 0, inside = 0, leaving = 0;
        for (size_t g = 0; g < G; g++) { hits += stats[g].edges; border += stats[g].borderline; inside += stats[g].inside; leaving += stats[g].leaving; }
        fprintf(stderr, "[timing] %u clusters of %zu genomes: %llu pairs inside, %llu leaving, from %llu hit records (%llu borderline)\n", n_cl, N, inside, leaving,
                hits, border);
    }
    rk_free_host(cl);
    j.leave();
}

// group: one sketch per cluster of a labelled collection (rk_group_sketches): its pan sketch (--pan, the default: the union of its
// members' sketches), its core sketch (--core: the hashes every member holds), the hashes at least P of Q of its members hold (--share
// P/Q), each with --min-count C (at least C members hold it) and --only (no genome outside the cluster holds it: its markers).  The
// labels come from --labels FILE (as medoid reads them) or from --by cluster|greedy|dbscan on the index this command builds anyway
// (default cluster at -D 0.05; dbscan with -m, default 5, leaves noise unlabelled).  out.sketch carries the input's info header and one
// sketch per cluster by ascending label, named after the member with the smallest index; --map: one line per cluster -- number from 1,
// label, genomes, hashes kept, name.  One GPU.
static int cmd_group(const Args &a)
{
    if (!a.has("o")) die("group needs -i and -o");
    SelfJoin j(a, "group", true);
    if (a.has("by") && a.has("labels")) die("command_group(), --by and --labels exclude each other: the labels come from one place");
    const string by = a.str("by", "cluster");
    if (by != "cluster" && by != "greedy" && by != "dbscan") die("command_group(), --by must be cluster, greedy or dbscan");
    if (a.num("gpus", 1) != 1) die("command_group(), group runs on one GPU (--gpus 1)");
    if ((int)a.has("pan") + (int)a.has("core") + (int)a.has("share") > 1) die("command_group(), --pan, --core and --share exclude each other");
    rk_group_rule rule{0, 1, 1, a.has("only") ? 1u : 0u};
    if (a.has("core")) rule.share_num = 1;
    if (a.has("share")) {
        const string sh = a.str("share", "");
        char *end = nullptr;
        const unsigned long long p = strtoull(sh.c_str(), &end, 10);
        const unsigned long long q = *end == '/' && end != sh.c_str() ? strtoull(end + 1, &end, 10) : 0;
        if (*end || !q || p > q || q > 0xFFFFFFFFULL || sh[0] == '-' || sh[0] == '+') die("command_group(), --share needs P/Q with 0 <= P <= Q and Q >= 1");
        rule.share_num = (uint32_t)p;
        rule.share_den = (uint32_t)q;
    }
    if (a.has("min-count")) {
        if (a.num("min-count", 0) < 1) die("command_group(), --min-count must be >= 1");
        rule.min_count = (uint32_t)a.num("min-count", 1);
    }
    const bool from_file = a.has("labels");
    const int min_pts = a.num("m", 5);
    if (!from_file && by == "dbscan" && min_pts < 1) die("command_group(), minPts must be >= 1\nUse -m to set the minPts (it counts the genome itself)");
    const double by_dist = a.real("D", 0.05);
    if (!from_file && 1.0 <= by_dist) die("command_group(), maxDist of --by must be below 1.0");
    j.prepare(1, false);
    const size_t N = j.N;
    Gpu &gpu = j.gpu(0);
    vector<uint32_t> label(N ? N : 1, RK_GROUP_NONE);
    if (from_file) {
        read_labels(a.str("labels", ""), N, "group", label);
    } else {
        rk_dist_opts o = j.opts(0);
        o.max_dist = by_dist;
        if (by == "cluster") {
            gpu.check(rk_cluster_rows(gpu.ctx, j.idx[0], &o, label.data(), nullptr), "rk_cluster_rows");
        } else if (by == "greedy") {
            rk_hit *links = nullptr;
            uint64_t n_links = 0;
            gpu.check(rk_greedy_rows(gpu.ctx, j.idx[0], &o, nullptr, label.data(), &links, &n_links, nullptr), "rk_greedy_rows");
            rk_free_host(links);
        } else {
            vector<uint8_t> kind(N ? N : 1);
            gpu.check(rk_dbscan_rows(gpu.ctx, j.idx[0], &o, (uint32_t)min_pts, label.data(), kind.data(), nullptr, nullptr, nullptr), "rk_dbscan_rows");
        }
    }
    if (getenv("RK_TIMING")) rk_ctx_set_timing(gpu.ctx, 1);
    rk_sketches *grouped = nullptr;
    uint32_t *group_label = nullptr, *group_size = nullptr, K = 0;
    rk_group_stats stats;
    gpu.check(rk_group_sketches(gpu.ctx, j.idx[0], label.data(), &rule, &grouped, &group_label, &group_size, &K, &stats), "rk_group_sketches");
    SketchSet out;
    out.info = j.s.info;
    out.off.assign((size_t)K + 1, 0);
    if (grouped) {
        if (out.wide()) {
            out.hashes64.resize(rk_sketches_total(grouped));
            gpu.check(rk_sketches_download64(grouped, out.hashes64.data(), out.off.data()), "rk_sketches_download64");
        } else {
            out.hashes.resize(rk_sketches_total(grouped));
            gpu.check(rk_sketches_download(grouped, out.hashes.data(), out.off.data()), "rk_sketches_download");
        }
    }
    j.phase_done("group sketches on the host", "grouping");
    {   // a group is named after its member with the smallest index
        vector<uint32_t> at(N ? N : 1, 0);
        for (uint32_t k = 0; k < K; k++) at[group_label[k]] = k;
        out.names.assign(K, string());
        vector<uint8_t> named(K ? K : 1, 0);
        for (size_t i = 0; i < N; i++)
            if (label[i] != RK_GROUP_NONE && !named[at[label[i]]]) {
                named[at[label[i]]] = 1;
                out.names[at[label[i]]] = j.s.names[i];
            }
    }
    string err;
    if (!save_sketches(j.out, out, err)) die("%s", err.c_str());
    if (a.has("map")) {
        FILE *mp = fopen(a.str("map", "").c_str(), "w");
        if (!mp) die("cannot write %s", a.str("map", "").c_str());
        for (uint32_t k = 0; k < K; k++)
            fprintf(mp, "%u\t%u\t%u\t%llu\t%s\n", k + 1, group_label[k], group_size[k], (unsigned long long)(out.off[k + 1] - out.off[k]), out.names[k].c_str());
        fclose(mp);
    }
    if (getenv("RK_TIMING"))
        fprintf(stderr, "[timing] %u group sketches of %u labelled genomes (%zu in all): %llu hashes kept from %llu lists (%llu by lane, %llu by wave, %llu by workgroup, %llu spilled), "
                        "%u attempt(s), path %u, %.3f ms on the device\n", K, stats.labelled, N, (unsigned long long)stats.kept, (unsigned long long)stats.lists,
                (unsigned long long)stats.lane_lists, (unsigned long long)stats.wave_lists, (unsigned long long)stats.block_lists, (unsigned long long)stats.spilled,
                stats.attempts, stats.path, rk_ctx_last_ms(gpu.ctx, RK_MS_GROUP));
    rk_free_host(group_label);
    rk_free_host(group_size);
    j.leave();
}

static int cmd_dist(const Args &a)
{
    if (!a.has("r") || !a.has("q")) die("dist needs -r and -q");
    const double max_dist = a.real("D", 1.0);
    if (max_dist < 0.0) die("command_dist(), maxDist must be > 0\nUse -D to set the maxDist");
    const int max_neighbor = a.num("N", 1);
    if (max_neighbor < 0) die("command_dist(), maxNeighbor must be > 0\nUse -N to set the maxNeighbor");
    const bool is_neighbor = a.has("N");
    const string out = a.str("o", "result.out");
    const int metric = a.num("M", 0);
    const int threads = a.num("t", (int)std::thread::hardware_concurrency());
    GpuSet set(a.num("device", 0), a.num("gpus", 1), a.has("same-device"));
    const double t_cmd0 = get_sec();
    SketchSet ref, qry;
    string ref_path, qry_path;
    {   // .sketch inputs are read while the runtime starts
        string err;
        if (is_sketch_file(a.str("r", ""))) {
            ref_path = a.str("r", "");
            if (!read_sketches(ref_path, ref, err)) die("readSketches(), %s", err.c_str());
        }
        if (is_sketch_file(a.str("q", ""))) {
            qry_path = a.str("q", "");
            if (!read_sketches(qry_path, qry, err)) die("readSketches(), %s", err.c_str());
        }
    }
    Gpu &gpu = set[0];
    if (ref_path.empty()) load_or_sketch(gpu, a.str("r", ""), a, threads, ref, ref_path);
    cerr << "the ref_sketch size is: " << ref.size() << endl;
    if (qry_path.empty()) load_or_sketch(gpu, a.str("q", ""), a, threads, qry, qry_path);
    if (qry.info.id != ref.info.id)  // src/subCommand.cpp:297-301
        die("command_dist(), the sketch infos between reference and query files are not match\n"
            "try to use the same shuffle file to generate sketches of the reference and query datasets");
    const bool missing = !exist_file(ref_path + ".index") || !exist_file(ref_path + ".dict");
    const size_t G = set.size();
    vector<rk_index *> idx(G, nullptr);
    build_everywhere(set, ref, ref_path, missing, idx);
    const double t1 = get_sec();
    cerr << "===================time of read index and offset sketch file is: " << t1 - t_cmd0 << endl;   // src/dist.cpp:482-485
    cerr << "=====total: " << qry.size() << endl;
    // contiguous query blocks: GPU g gets queries [q0[g], q0[g+1]) as a sketch set of its own (the host scatters the
    // queries) and reports rows relative to it
    const uint32_t Q = (uint32_t)qry.size();
    vector<uint32_t> q0(G + 1, Q);
    for (size_t g = 0; g <= G; g++) q0[g] = (uint32_t)((uint64_t)Q * g / G);
    vector<rk_hit *> hits(G, nullptr);
    vector<uint64_t> n_hits(G, 0);
    auto rows_of = [&](size_t g) {
        Gpu &dev = set[g];
        const uint32_t nq = q0[g + 1] - q0[g];
        vector<uint64_t> off(nq + 1);
        for (uint32_t i = 0; i <= nq; i++) off[i] = qry.off[q0[g] + i] - qry.off[q0[g]];
        rk_sketches *qs = nullptr;
        if (qry.wide())
            dev.check(rk_sketches_from_host64(dev.ctx, qry.hashes64.data() + qry.off[q0[g]], off.data(), nq, &qs), "rk_sketches_from_host64");
        else
            dev.check(rk_sketches_from_host(dev.ctx, qry.hashes.data() + qry.off[q0[g]], off.data(), nq, &qs), "rk_sketches_from_host");
        rk_dist_opts o{};
        o.triangle = 0;
        o.metric = metric;
        o.kmer_size = 2 * ref.info.half_k;
        o.max_dist = max_dist;
        if (is_neighbor)   // -N: the nearest references per query row (src/dist.cpp:599,625-640), never all Q x R pairs
            dev.check(rk_dist_topn(dev.ctx, idx[g], qs, &o, (uint64_t)max_neighbor, &hits[g], &n_hits[g]), "rk_dist_topn");
        else
            dev.check(rk_dist_rows(dev.ctx, idx[g], qs, &o, &hits[g], &n_hits[g], nullptr), "rk_dist_rows");
        for (uint64_t i = 0; i < n_hits[g]; i++) hits[g][i].row += q0[g];
        rk_sketches_free(qs);
    };
    on_every_gpu(G, rows_of);
    cerr << "===================time of multiple threads distance computing and save the subFile is: " << get_sec() - t1 << endl;
    vector<HitPart> parts(G);
    for (size_t g = 0; g < G; g++) {
        parts[g].hits = hits[g];
        parts[g].n = n_hits[g];
        for (uint32_t r = q0[g]; r < q0[g + 1]; r++) parts[g].rows.push_back(r);
    }
    write_hits(out, parts, false, qry.names, ref.names, threads);
    for (size_t g = 0; g < G; g++) {
        rk_free_host(hits[g]);
        rk_index_free(idx[g]);
    }
    return 0;
}

// assign: placement of the queries into the clustered references (rk_assign_rows).  The reference index is replicated on every GPU as
// dist --gpus does; every GPU places the query rows dealt to it (blocks of 32, round-robin) and writes them into ONE set of arrays: a
// query's result depends on its own records alone, so nothing is merged.  The references' labels come from --labels FILE (the format of
// medoid --labels) or from --by on the same index with the same -D and -M: cluster (the default; rk_cluster_rows, its rows dealt to the
// GPUs), greedy (rk_greedy_rows) or dbscan -m minPts (rk_dbscan_rows; the non-core references become unlabelled: DBSCAN's "predict"), the
// last two on the first GPU.  One line per query in input order: its name, the name of the genome whose index is its label, the nearest
// labelled reference's name, common|size0|size1, jorc and dist as dist prints them, its references of that label, its labelled
// references and all its references within -D, the name of the runner-up cluster and the distance of its nearest member (- -
// without one); a novel query has - in the five fields behind its name.  --novel: the names of the novel queries.
static int cmd_assign(const Args &a)
{
    if (!a.has("r") || !a.has("q")) die("assign needs -r and -q");
    if (!a.has("D")) die("command_assign(), assign needs -D: the distance within which a reference anchors a query");
    const double max_dist = a.real("D", 1.0);
    if (max_dist < 0.0) die("command_assign(), maxDist must be > 0\nUse -D to set the maxDist");
    if (!(max_dist < 1.0)) die("command_assign(), maxDist must stay below 1.0: at 1.0 every reference is within -D of every query (a dense report), and pairs that share nothing carry no order");
    const string by = a.str("by", "cluster");
    if (a.has("by") && a.has("labels")) die("command_assign(), --by and --labels exclude each other: the labels come from one place");
    if (by != "cluster" && by != "greedy" && by != "dbscan") die("command_assign(), --by must be cluster, greedy or dbscan");
    const bool from_file = a.has("labels");
    if (!from_file && by == "dbscan" && (!a.has("m") || a.num("m", 0) < 1))
        die("command_assign(), minPts must be >= 1\nUse -m to set the minPts (it counts the genome itself)");
    const string out = a.str("o", "result.out");
    const int metric = a.num("M", 0);
    const int threads = a.num("t", (int)std::thread::hardware_concurrency());
    GpuSet set(a.num("device", 0), a.num("gpus", 1), a.has("same-device"));
    const double t_cmd0 = get_sec();
    SketchSet ref, qry;
    string ref_path, qry_path;
    {   // .sketch inputs are read while the runtime starts
        string err;
        if (is_sketch_file(a.str("r", ""))) {
            ref_path = a.str("r", "");
            if (!read_sketches(ref_path, ref, err)) die("readSketches(), %s", err.c_str());
        }
        if (is_sketch_file(a.str("q", ""))) {
            qry_path = a.str("q", "");
            if (!read_sketches(qry_path, qry, err)) die("readSketches(), %s", err.c_str());
        }
    }
    if (ref_path.empty()) load_or_sketch(set[0], a.str("r", ""), a, threads, ref, ref_path);
    cerr << "the ref_sketch size is: " << ref.size() << endl;
    if (qry_path.empty()) load_or_sketch(set[0], a.str("q", ""), a, threads, qry, qry_path);
    if (qry.info.id != ref.info.id)
        die("command_assign(), the sketch infos between reference and query files are not match\n"
            "try to use the same shuffle file to generate sketches of the reference and query datasets");
    const size_t G = set.size(), N = ref.size(), Q = qry.size();
    vector<uint32_t> label(N ? N : 1, RK_ASSIGN_NONE);
    if (from_file) read_labels(a.str("labels", ""), N, "assign", label);   // (before the index: a bad file costs no build)
    const bool missing = !exist_file(ref_path + ".index") || !exist_file(ref_path + ".dict");
    vector<rk_index *> idx(G, nullptr);
    build_everywhere(set, ref, ref_path, missing, idx);
    stamp("index built");
    const double t1 = get_sec();
    cerr << "===================time of read index and offset sketch file is: " << t1 - t_cmd0 << endl;
    cerr << "=====total: " << Q << endl;
    auto opts_of = [&](size_t g, int triangle) {   // GPU g's rows: of the self join that labels the references, or of the queries
        rk_dist_opts o{};
        o.triangle = triangle;
        o.metric = metric;
        o.kmer_size = 2 * ref.info.half_k;
        o.max_dist = max_dist;
        if (G > 1) {
            o.row_first = (uint32_t)g;
            o.row_step = (uint32_t)G;
            o.row_block = kRowBlock;
        }
        return o;
    };
    if (!from_file && N) {
        if (by == "cluster") {
            vector<vector<uint32_t>> labels(G, vector<uint32_t>(N));
            on_every_gpu(G, [&](size_t g) {
                const rk_dist_opts o = opts_of(g, 1);
                set[g].check(rk_cluster_rows(set[g].ctx, idx[g], &o, labels[g].data(), nullptr), "rk_cluster_rows");
            });
            for (size_t g = 1; g < G; g++)
                if (rk_cluster_merge(labels[0].data(), labels[g].data(), (uint32_t)N, labels[0].data()) != 0) die("rk_cluster_merge failed");
            label = labels[0];
        } else {
            rk_dist_opts o = opts_of(0, 1);
            o.row_first = 0;   // every row on the first GPU: neither rule composes from shards
            o.row_step = 1;
            o.row_block = 0;
            if (by == "greedy") {
                rk_hit *links = nullptr;
                uint64_t n_links = 0;
                set[0].check(rk_greedy_rows(set[0].ctx, idx[0], &o, nullptr, label.data(), &links, &n_links, nullptr), "rk_greedy_rows");
                rk_free_host(links);
            } else {
                vector<uint8_t> kind(N);
                set[0].check(rk_dbscan_rows(set[0].ctx, idx[0], &o, (uint32_t)a.num("m", 1), label.data(), kind.data(), nullptr, nullptr, nullptr), "rk_dbscan_rows");
                for (size_t i = 0; i < N; i++)
                    if (kind[i] != 2) label[i] = RK_ASSIGN_NONE;   // only a core reference anchors a query
            }
        }
        stamp("references labelled");
    }
    // one set of arrays for all GPUs: each writes the entries of its rows
    const size_t Qa = Q ? Q : 1;
    vector<uint32_t> q_label(Qa, RK_ASSIGN_NONE), n_within(Qa, 0), n_labelled(Qa, 0), n_same(Qa, 0);
    vector<rk_hit> nearest(Qa), runner_up(Qa);
    rk_assign_queries res{q_label.data(), n_within.data(), n_labelled.data(), n_same.data(), nearest.data(), runner_up.data()};
    vector<rk_assign_stats> stats(G);
    on_every_gpu(G, [&](size_t g) {
        Gpu &dev = set[g];
        rk_sketches *qs = upload(dev, qry);
        const rk_dist_opts o = opts_of(g, 0);
        dev.check(rk_assign_rows(dev.ctx, idx[g], qs, &o, label.data(), &res, &stats[g]), "rk_assign_rows");
        rk_sketches_free(qs);
    });
    stamp("queries placed");
    cerr << "===================time of multiple threads distance computing and placement is: " << get_sec() - t1 << endl;
    FILE *fp = fopen(out.c_str(), "w");
    if (!fp) die("cannot write %s", out.c_str());
    FILE *np = nullptr;
    if (a.has("novel") && !(np = fopen(a.str("novel", "").c_str(), "w"))) die("cannot write %s", a.str("novel", "").c_str());
    for (size_t q = 0; q < Q; q++) {
        const rk_hit &h = nearest[q], &s = runner_up[q];
        if (q_label[q] == RK_ASSIGN_NONE) {
            fprintf(fp, "%s\t-\t-\t-\t-\t-\t%u\t%u\t%u\t-\t-\n", qry.names[q].c_str(), n_same[q], n_labelled[q], n_within[q]);
            if (np) fprintf(np, "%s\n", qry.names[q].c_str());
            continue;
        }
        fprintf(fp, "%s\t%s\t%s\t%d|%d|%d\t%f\t%f\t%u\t%u\t%u\t", qry.names[q].c_str(), ref.names[q_label[q]].c_str(), ref.names[h.col].c_str(), h.common, h.size0,
                h.size1, h.jorc, h.dist, n_same[q], n_labelled[q], n_within[q]);
        if (s.row == RK_ASSIGN_NONE) fprintf(fp, "-\t-\n");
        else fprintf(fp, "%s\t%f\n", ref.names[label[s.col]].c_str(), s.dist);
    }
    fclose(fp);
    if (np) fclose(np);
    if (getenv("RK_TIMING")) {
        unsigned long long hits = 0, border = 0, placed = 0, novel = 0, ambiguous = 0;
        for (size_t g = 0; g < G; g++) { hits += stats[g].edges; border += stats[g].borderline; placed += stats[g].placed; novel += stats[g].novel; ambiguous += stats[g].ambiguous; }
        fprintf(stderr, "[timing] %zu queries against %zu references: %llu placed (%llu with a runner-up), %llu novel, from %llu hit records (%llu borderline)\n", Q, N,
                placed, ambiguous, novel, hits, border);
    }
    SelfJoin::leave();
}

// the sketches of `qry` on the device with only the hashes that between rule.min_refs and rule.max_refs sketches of `ref` hold
// (rk_sketches_mask); NULL without a query sketch.  The index of `ref` is built for the call, and written next to ref_path when asked.
// counted: the queries go up with qry.counts and every survivor keeps its count (rk_sketches_mask_counts).
static rk_sketches *masked_queries(GpuSet &set, const SketchSet &ref, const string &ref_path, bool write_files, const SketchSet &qry, const rk_mask_rule &rule,
                                   rk_mask_stats *stats, bool counted = false)
{
    vector<rk_index *> idx(1, nullptr);
    build_everywhere(set, ref, ref_path, write_files, idx);
    rk_sketches *qs = counted ? upload_counted(set[0], qry) : upload(set[0], qry), *out = nullptr;
    if (counted) set[0].check(rk_sketches_mask_counts(set[0].ctx, qs, idx[0], &rule, &out, stats), "rk_sketches_mask_counts");
    else set[0].check(rk_sketches_mask(set[0].ctx, qs, idx[0], &rule, &out, stats), "rk_sketches_mask");
    rk_sketches_free(qs);
    rk_index_free(idx[0]);
    return out;
}

// mask: the query sketches with only the hashes that between --min-refs and --max-refs reference sketches hold (rk_sketches_mask).
// --keep absent (the default, {0, 0}) writes the sketches `sub` writes, with the hashes of every sketch ascending; --keep present
// ({1, no limit}) the intersection.  out.sketch: the queries' info and names, one sketch per query in input order.
static int cmd_mask(const Args &a)
{
    if (!a.has("r") || !a.has("q") || !a.has("o")) die("mask needs -r, -q and -o");
    if (a.num("gpus", 1) != 1) die("command_mask(), mask runs on one GPU (--gpus 1)");
    if (a.has("keep") && (a.has("min-refs") || a.has("max-refs"))) die("command_mask(), --keep and --min-refs / --max-refs exclude each other");
    const string keep = a.str("keep", "absent");
    if (keep != "absent" && keep != "present") die("command_mask(), --keep must be absent or present");
    need_sketch_queries(a, "mask");
    rk_mask_rule rule{0, 0};
    if (keep == "present") rule = rk_mask_rule{1, 0xFFFFFFFFu};
    if (a.has("min-refs") || a.has("max-refs")) {
        auto bound = [&](const char *key, uint32_t otherwise) {
            if (!a.has(key)) return otherwise;
            const string v = a.str(key, "");
            char *end = nullptr;
            const unsigned long long x = strtoull(v.c_str(), &end, 10);
            if (v.empty() || *end || v[0] == '-' || v[0] == '+' || x > 0xFFFFFFFFULL) die("command_mask(), --%s needs an integer from 0 to 4294967295", key);
            return (uint32_t)x;
        };
        rule.min_refs = bound("min-refs", 0u);
        rule.max_refs = bound("max-refs", 0xFFFFFFFFu);
        if (rule.min_refs > rule.max_refs) die("command_mask(), --min-refs must not exceed --max-refs");
    }
    const int threads = a.num("t", (int)std::thread::hardware_concurrency());
    GpuSet set(a.num("device", 0), 1, false);
    SketchSet ref, qry;
    string ref_path, qry_path;
    {   // .sketch inputs are read while the runtime starts
        string err;
        if (is_sketch_file(a.str("r", ""))) {
            ref_path = a.str("r", "");
            if (!read_sketches(ref_path, ref, err)) die("readSketches(), %s", err.c_str());
        }
        if (is_sketch_file(a.str("q", ""))) {
            qry_path = a.str("q", "");
            if (!read_sketches(qry_path, qry, err)) die("readSketches(), %s", err.c_str());
        }
    }
    if (ref_path.empty()) load_or_sketch(set[0], a.str("r", ""), a, threads, ref, ref_path);
    cerr << "the ref_sketch size is: " << ref.size() << endl;
    if (qry_path.empty()) load_or_sketch(set[0], a.str("q", ""), a, threads, qry, qry_path);
    if (qry.info.id != ref.info.id)
        die("command_mask(), the sketch infos between reference and query files are not match\n"
            "try to use the same shuffle file to generate sketches of the reference and query datasets");
    const bool abund = a.has("abund");   // --abund: the counts of the queries go along, into out.sketch.abund
    if (abund) need_counted_queries("mask", qry_path, qry);
    // the .dict/.index pair next to the reference is (re)written only if missing, as dist does
    const bool missing = !exist_file(ref_path + ".index") || !exist_file(ref_path + ".dict");
    if (getenv("RK_TIMING")) rk_ctx_set_timing(set[0].ctx, 1);
    rk_mask_stats stats;
    rk_sketches *kept = masked_queries(set, ref, ref_path, missing, qry, rule, &stats, abund);
    stamp("queries masked");
    SketchSet out;
    out.info = qry.info;
    out.names = qry.names;
    out.off.assign(qry.size() + 1, 0);
    if (kept) {
        if (out.wide()) {
            out.hashes64.resize(rk_sketches_total(kept));
            set[0].check(rk_sketches_download64(kept, out.hashes64.data(), out.off.data()), "rk_sketches_download64");
        } else {
            out.hashes.resize(rk_sketches_total(kept));
            set[0].check(rk_sketches_download(kept, out.hashes.data(), out.off.data()), "rk_sketches_download");
        }
        if (abund) {
            out.counts.resize(rk_sketches_total(kept));
            set[0].check(rk_sketches_download_counts(kept, out.counts.data()), "rk_sketches_download_counts");
        }
        rk_sketches_free(kept);
    }
    string err;
    if (!save_sketches(a.str("o", ""), out, err)) die("%s", err.c_str());
    if (abund && !save_abund(abund_path(a.str("o", "")), out, err)) die("%s", err.c_str());
    if (getenv("RK_TIMING"))
        fprintf(stderr, "[timing] %zu queries against %zu references: %llu of %llu hashes kept (%llu have a posting list), %u sketches emptied, %llu tiles, %u scan block(s), "
                        "path %u, %.3f ms on the device\n", qry.size(), ref.size(), (unsigned long long)stats.kept, (unsigned long long)stats.hashes,
                (unsigned long long)stats.matched, stats.emptied, (unsigned long long)stats.tiles, stats.scan_blocks, stats.path, rk_ctx_last_ms(set[0].ctx, RK_MS_MASK));
    SelfJoin::leave();
}

// gather: which references explain each query sketch (rk_gather_rows): per round the reference that holds most of the query's hashes
// no earlier pick held -- the greedy minimum set cover, a metagenome's decomposition.  One line per pick:
// query, reference, rank, common|size_ref|size_query, fresh, fresh / size_query, common / size_ref.
// --sub host.sketch: the queries lose the hashes of host.sketch on the device first (rk_sketches_mask {0, 0}): the cover of what `sub` would leave.
static int cmd_gather(const Args &a)
{
    if (!a.has("r") || !a.has("q")) die("gather needs -r and -q");
    if (a.num("gpus", 1) != 1) die("command_gather(), gather runs on one GPU (--gpus 1)");
    if (a.has("min-new") && a.num("min-new", 1) < 1) die("command_gather(), --min-new must be >= 1");
    if (a.has("max-picks") && a.num("max-picks", 0) < 0) die("command_gather(), --max-picks must be >= 0 (0: no limit)");
    const string out = a.str("o", "result.out");
    const int threads = a.num("t", (int)std::thread::hardware_concurrency());
    GpuSet set(a.num("device", 0), 1, false);
    SketchSet ref, qry;
    string ref_path, qry_path;
    {   // .sketch inputs are read while the runtime starts
        string err;
        if (is_sketch_file(a.str("r", ""))) {
            ref_path = a.str("r", "");
            if (!read_sketches(ref_path, ref, err)) die("readSketches(), %s", err.c_str());
        }
        if (is_sketch_file(a.str("q", ""))) {
            qry_path = a.str("q", "");
            if (!read_sketches(qry_path, qry, err)) die("readSketches(), %s", err.c_str());
        }
    }
    if (ref_path.empty()) load_or_sketch(set[0], a.str("r", ""), a, threads, ref, ref_path);
    cerr << "the ref_sketch size is: " << ref.size() << endl;
    if (qry_path.empty()) load_or_sketch(set[0], a.str("q", ""), a, threads, qry, qry_path);
    if (qry.info.id != ref.info.id)
        die("command_gather(), the sketch infos between reference and query files are not match\n"
            "try to use the same shuffle file to generate sketches of the reference and query datasets");
    const size_t N = ref.size(), Q = qry.size();
    const bool missing = !exist_file(ref_path + ".index") || !exist_file(ref_path + ".dict");
    vector<rk_index *> idx(1, nullptr);
    build_everywhere(set, ref, ref_path, missing, idx);
    stamp("index built");
    cerr << "=====total: " << Q << endl;
    const rk_gather_opts o{(uint32_t)a.num("min-new", 1), (uint32_t)a.num("max-picks", 0), 0, 0, 0};
    vector<uint64_t> off(Q + 1, 0);
    vector<uint32_t> matched(Q ? Q : 1, 0), n_cand(Q ? Q : 1, 0), covered(Q ? Q : 1, 0);
    rk_gather_pick *picks = nullptr;
    uint64_t n_picks = 0;
    rk_gather_stats stats;
    rk_sketches *qs = nullptr;
    vector<uint64_t> q_off = qry.off;   // the sizes of the queries as they are covered
    if (a.has("sub")) {
        const string host_path = a.str("sub", "");
        if (!is_sketch_file(host_path)) die("command_gather(), %s is not sketch file, --sub needs a sketch file", host_path.c_str());
        SketchSet host;
        string err;
        if (!read_sketches(host_path, host, err)) die("readSketches(), %s", err.c_str());
        if (host.info.id != qry.info.id) die("command_gather(), the sketch infos between the --sub sketches and the query sketches are not same");
        qs = masked_queries(set, host, host_path, false, qry, rk_mask_rule{0, 0}, nullptr);
        if (qs) set[0].check(rk_sketches_download(qs, nullptr, q_off.data()), "rk_sketches_download");
        stamp("queries masked");
    }
    if (!qs) qs = upload(set[0], qry);
    set[0].check(rk_gather_rows(set[0].ctx, idx[0], qs, &o, off.data(), &picks, &n_picks, matched.data(), n_cand.data(), covered.data(), &stats), "rk_gather_rows");
    rk_sketches_free(qs);
    stamp("queries decomposed");
    FILE *fp = fopen(out.c_str(), "w");
    if (!fp) die("cannot write %s", out.c_str());
    for (uint64_t k = 0; k < n_picks; k++) {
        const rk_gather_pick &p = picks[k];
        fprintf(fp, "%s\t%s\t%u\t%u|%u|%u\t%u\t%f\t%f\n", qry.names[p.query].c_str(), ref.names[p.ref].c_str(), p.rank, p.common, p.size_ref, p.size_query, p.fresh,
                (double)p.fresh / (double)p.size_query, (double)p.common / (double)p.size_ref);
    }
    fclose(fp);
    if (a.has("summary")) {
        FILE *sp = fopen(a.str("summary", "").c_str(), "w");
        if (!sp) die("cannot write %s", a.str("summary", "").c_str());
        for (size_t q = 0; q < Q; q++)
            fprintf(sp, "%s\t%llu\t%u\t%u\t%u\t%llu\n", qry.names[q].c_str(), (unsigned long long)(q_off[q + 1] - q_off[q]), matched[q], covered[q], n_cand[q],
                    (unsigned long long)(off[q + 1] - off[q]));
        fclose(sp);
    }
    if (getenv("RK_TIMING"))
        fprintf(stderr, "[timing] %zu queries against %zu references: %llu picks of %llu candidates in %u rounds (%u launched, %u batches, %u read-backs), %llu lists died "
                        "(%llu by lane, %llu by wave, %llu by workgroup), path %u\n", Q, N, (unsigned long long)stats.picks, (unsigned long long)stats.candidates, stats.rounds,
                stats.launched_rounds, stats.batches, stats.read_backs, (unsigned long long)(stats.lane_lists + stats.wave_lists + stats.block_lists),
                (unsigned long long)stats.lane_lists, (unsigned long long)stats.wave_lists, (unsigned long long)stats.block_lists, stats.path);
    rk_free_host(picks);
    SelfJoin::leave();
}

// screen: which references are contained in each query sketch, every shared hash credited to one reference only (rk_screen_rows): the
// winner-take-all containment screen of `mash screen -w`.  One line per record: query, reference, common, size_ref, won,
// identity = (common / size_ref)^(1/K), identity_won = (won / size_ref)^(1/K), K the k-mer length of the sketches.
// --sub host.sketch: the queries lose the hashes of host.sketch on the device first (rk_sketches_mask {0, 0}), as gather --sub does.
static int cmd_screen(const Args &a)
{
    if (!a.has("r") || !a.has("q")) die("screen needs -r and -q");
    if (a.num("gpus", 1) != 1) die("command_screen(), screen runs on one GPU (--gpus 1)");
    if (a.has("min-common") && a.num("min-common", 1) < 1) die("command_screen(), --min-common must be >= 1");
    if (a.has("min-won") && a.num("min-won", 0) < 0) die("command_screen(), --min-won must be >= 0 (0: every candidate)");
    need_sketch_queries(a, "screen");
    const string out = a.str("o", "result.out");
    const int threads = a.num("t", (int)std::thread::hardware_concurrency());
    GpuSet set(a.num("device", 0), 1, false);
    SketchSet ref, qry;
    string ref_path, qry_path;
    {   // .sketch inputs are read while the runtime starts
        string err;
        if (is_sketch_file(a.str("r", ""))) {
            ref_path = a.str("r", "");
            if (!read_sketches(ref_path, ref, err)) die("readSketches(), %s", err.c_str());
        }
        if (is_sketch_file(a.str("q", ""))) {
            qry_path = a.str("q", "");
            if (!read_sketches(qry_path, qry, err)) die("readSketches(), %s", err.c_str());
        }
    }
    if (ref_path.empty()) load_or_sketch(set[0], a.str("r", ""), a, threads, ref, ref_path);
    cerr << "the ref_sketch size is: " << ref.size() << endl;
    if (qry_path.empty()) load_or_sketch(set[0], a.str("q", ""), a, threads, qry, qry_path);
    if (qry.info.id != ref.info.id)
        die("command_screen(), the sketch infos between reference and query files are not match\n"
            "try to use the same shuffle file to generate sketches of the reference and query datasets");
    const bool abund = a.has("abund");   // --abund: four more columns per line, three more per line of --summary (rk_screen_abund_rows)
    if (abund) need_counted_queries("screen", qry_path, qry);
    const size_t N = ref.size(), Q = qry.size();
    const bool missing = !exist_file(ref_path + ".index") || !exist_file(ref_path + ".dict");
    vector<rk_index *> idx(1, nullptr);
    build_everywhere(set, ref, ref_path, missing, idx);
    stamp("index built");
    cerr << "=====total: " << Q << endl;
    const rk_screen_opts o{(uint32_t)a.num("min-common", 1), (uint32_t)a.num("min-won", 0), 0, 0, 0};
    vector<uint64_t> off(Q + 1, 0);
    vector<uint32_t> matched(Q ? Q : 1, 0), n_cand(Q ? Q : 1, 0), claimed(Q ? Q : 1, 0);
    rk_screen_rec *recs = nullptr;
    rk_screen_abund *abunds = nullptr;
    vector<uint64_t> occ(abund ? 3 * Q + 1 : 1, 0);
    uint64_t n_recs = 0;
    rk_screen_stats stats;
    rk_screen_abund_stats abund_stats;
    rk_sketches *qs = nullptr;
    vector<uint64_t> q_off = qry.off;   // the sizes of the queries as they are screened
    if (a.has("sub")) {
        const string host_path = a.str("sub", "");
        if (!is_sketch_file(host_path)) die("command_screen(), %s is not sketch file, --sub needs a sketch file", host_path.c_str());
        SketchSet host;
        string err;
        if (!read_sketches(host_path, host, err)) die("readSketches(), %s", err.c_str());
        if (host.info.id != qry.info.id) die("command_screen(), the sketch infos between the --sub sketches and the query sketches are not same");
        qs = masked_queries(set, host, host_path, false, qry, rk_mask_rule{0, 0}, nullptr, abund);
        if (qs) set[0].check(rk_sketches_download(qs, nullptr, q_off.data()), "rk_sketches_download");
        stamp("queries masked");
    }
    if (!qs) qs = abund ? upload_counted(set[0], qry) : upload(set[0], qry);
    if (abund) {
        set[0].check(rk_screen_abund_rows(set[0].ctx, idx[0], qs, &o, off.data(), &recs, &abunds, &n_recs, matched.data(), n_cand.data(), claimed.data(), occ.data(),
                                          &abund_stats), "rk_screen_abund_rows");
        memcpy(&stats, &abund_stats, sizeof stats);   // (rk_screen_abund_stats begins with rk_screen_stats)
    } else {
        set[0].check(rk_screen_rows(set[0].ctx, idx[0], qs, &o, off.data(), &recs, &n_recs, matched.data(), n_cand.data(), claimed.data(), &stats), "rk_screen_rows");
    }
    rk_sketches_free(qs);
    stamp("queries screened");
    const double inv_k = 1.0 / (double)(2 * ref.info.half_k);   // the k-mer length, as dist reads it
    FILE *fp = fopen(out.c_str(), "w");
    if (!fp) die("cannot write %s", out.c_str());
    for (uint64_t k = 0; k < n_recs; k++) {
        const rk_screen_rec &p = recs[k];
        fprintf(fp, "%s\t%s\t%u\t%u\t%u\t%.6f\t%.6f", qry.names[p.query].c_str(), ref.names[p.ref].c_str(), p.common, p.size_ref, p.won,
                pow((double)p.common / (double)p.size_ref, inv_k), p.won ? pow((double)p.won / (double)p.size_ref, inv_k) : 0.0);
        if (abund)   // the lower median and the mean count over what the record shares, then over what it claims
            fprintf(fp, "\t%u\t%.3f\t%u\t%.3f", abunds[k].med_common, (double)abunds[k].occ_common / (double)p.common, abunds[k].med_won,
                    p.won ? (double)abunds[k].occ_won / (double)p.won : 0.0);
        fputc('\n', fp);
    }
    fclose(fp);
    if (a.has("summary")) {
        FILE *sp = fopen(a.str("summary", "").c_str(), "w");
        if (!sp) die("cannot write %s", a.str("summary", "").c_str());
        for (size_t q = 0; q < Q; q++) {
            fprintf(sp, "%s\t%llu\t%u\t%u\t%u\t%llu", qry.names[q].c_str(), (unsigned long long)(q_off[q + 1] - q_off[q]), matched[q], n_cand[q], claimed[q],
                    (unsigned long long)(off[q + 1] - off[q]));
            if (abund)   // the sums of the counts over the whole sketch, over its matched and over its claimed hashes
                fprintf(sp, "\t%llu\t%llu\t%llu", (unsigned long long)occ[3 * q], (unsigned long long)occ[3 * q + 1], (unsigned long long)occ[3 * q + 2]);
            fputc('\n', sp);
        }
        fclose(sp);
    }
    if (getenv("RK_TIMING"))
        fprintf(stderr, "[timing] %zu queries against %zu references: %llu records of %llu candidates, %llu of %llu matched hashes claimed, %llu postings walked "
                        "(%llu lists by lane, %llu by wave, %llu by workgroup), %llu adds, %u batches, %u launches, %u read-backs, path %u, %.3f ms on the device\n",
                Q, N, (unsigned long long)stats.records, (unsigned long long)stats.candidates, (unsigned long long)stats.claimed, (unsigned long long)stats.matched,
                (unsigned long long)stats.postings_walked, (unsigned long long)stats.lane_lists, (unsigned long long)stats.wave_lists,
                (unsigned long long)stats.block_lists, (unsigned long long)stats.adds, stats.batches, stats.launches, stats.read_backs, stats.path,
                rk_ctx_last_ms(set[0].ctx, abund ? RK_MS_SCREEN_ABUND : RK_MS_SCREEN));
    rk_free_host(recs);
    rk_free_host(abunds);
    SelfJoin::leave();
}

// --taxonomy FILE of lca: one line per node, id<TAB>parent id[<TAB>name]; ids are arbitrary non-negative integers (NCBI taxids work),
// the root names itself.  The nodes become dense numbers by ascending id: id[] ascending, parent[] in node numbers, name[] ("" without).
struct Taxonomy {
    vector<unsigned long long> id;
    vector<uint32_t> parent;
    vector<string> name;
    // the node number of an id, or -1
    long long node_of(unsigned long long x) const
    {
        const auto it = std::lower_bound(id.begin(), id.end(), x);
        return it != id.end() && *it == x ? (long long)(it - id.begin()) : -1;
    }
};

static bool parse_id(const string &s, unsigned long long &out)
{
    // digits only (strtoull would take white space and a sign), and no more than 64 bits hold
    if (s.empty() || s.size() > 20 || s.find_first_not_of("0123456789") != string::npos) return false;
    errno = 0;
    out = strtoull(s.c_str(), nullptr, 10);
    return errno == 0;
}

static void read_taxonomy(const string &path, Taxonomy &t)
{
    std::ifstream in(path);
    if (!in) die("cannot read %s", path.c_str());
    struct Row { unsigned long long id, parent; string name; };
    vector<Row> rows;
    string line;
    size_t n = 0;
    while (std::getline(in, line)) {
        n++;
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (line.empty()) continue;
        const size_t t1 = line.find('\t'), t2 = t1 == string::npos ? string::npos : line.find('\t', t1 + 1);
        Row r;
        if (t1 == string::npos || !parse_id(line.substr(0, t1), r.id) || !parse_id(line.substr(t1 + 1, t2 == string::npos ? string::npos : t2 - t1 - 1), r.parent))
            die("command_lca(), line %zu of %s is not id<TAB>parent id[<TAB>name] with non-negative integers", n, path.c_str());
        if (t2 != string::npos) r.name = line.substr(t2 + 1);
        rows.push_back(r);
    }
    if (rows.empty()) die("command_lca(), %s holds no node", path.c_str());
    if (rows.size() >= 0x80000000ULL) die("command_lca(), %s holds 2^31 nodes or more", path.c_str());
    std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) { return a.id < b.id; });
    for (size_t k = 1; k < rows.size(); k++)
        if (rows[k].id == rows[k - 1].id) die("command_lca(), %s names the node %llu twice", path.c_str(), rows[k].id);
    for (const Row &r : rows) {
        t.id.push_back(r.id);
        t.name.push_back(r.name);
    }
    size_t roots = 0;
    for (const Row &r : rows) {
        const long long p = t.node_of(r.parent);
        if (p < 0) die("command_lca(), the parent %llu of node %llu is no node of %s", r.parent, r.id, path.c_str());
        t.parent.push_back((uint32_t)p);
        roots += r.parent == r.id;
    }
    if (roots != 1) die("command_lca(), %s holds %zu roots (a node that names itself as its parent): exactly one is needed", path.c_str(), roots);
}

// --taxa FILE of lca: one line per reference in input order, an id of the taxonomy or - for an unlabelled reference
static void read_taxa(const string &path, size_t N, const Taxonomy &t, vector<uint32_t> &taxa)
{
    std::ifstream in(path);
    if (!in) die("cannot read %s", path.c_str());
    string line;
    size_t seen = 0;
    while (std::getline(in, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (line.empty() && in.peek() == EOF) break;
        if (seen >= N) die("command_lca(), %s holds more than the %zu lines of the input", path.c_str(), N);
        if (line != "-") {
            unsigned long long v = 0;
            const long long node = parse_id(line, v) ? t.node_of(v) : -1;
            if (node < 0) die("command_lca(), line %zu of %s is neither an id of the taxonomy nor -", seen + 1, path.c_str());
            taxa[seen] = (uint32_t)node;
        }
        seen++;
    }
    if (seen != N) die("command_lca(), %s holds %zu lines, the input %zu genomes", path.c_str(), seen, N);
}

// lca: every query classified by the per-hash lowest common ancestor in a taxonomy over the references (rk_lca_rows, rk_lca_call).
// One line per query: name, called id or -, its name, candidate id, clade, retained, matched, unlabelled, sketch size.
// --summary: one line per record of a query's tally: query, id, name, direct, clade.
static int cmd_lca(const Args &a)
{
    if (!a.has("r") || !a.has("q") || !a.has("o") || !a.has("taxonomy") || !a.has("taxa")) die("lca needs -r, -q, --taxonomy, --taxa and -o");
    if (a.num("gpus", 1) != 1) die("command_lca(), lca runs on one GPU (--gpus 1)");
    rk_lca_rule rule{1, 0, 1, 0};
    if (a.has("min-count")) {
        unsigned long long v = 0;
        if (!parse_id(a.str("min-count", ""), v) || v < 1 || v > 0xFFFFFFFFULL) die("command_lca(), --min-count needs an integer from 1 to 4294967295");
        rule.min_count = (uint32_t)v;
    }
    if (a.has("confidence")) {
        const string c = a.str("confidence", "");
        const size_t slash = c.find('/');
        unsigned long long p = 0, q = 0;
        if (slash == string::npos || !parse_id(c.substr(0, slash), p) || !parse_id(c.substr(slash + 1), q) || !q || p > q || q > 0xFFFFFFFFULL)
            die("command_lca(), --confidence needs P/Q with 0 <= P <= Q and Q >= 1");
        rule.conf_num = (uint32_t)p;
        rule.conf_den = (uint32_t)q;
    }
    const string of = a.str("of", "labelled");
    if (of != "labelled" && of != "sketch") die("command_lca(), --of must be labelled or sketch");
    rule.denom = of == "sketch";
    Taxonomy tax;
    read_taxonomy(a.str("taxonomy", ""), tax);
    const int threads = a.num("t", (int)std::thread::hardware_concurrency());
    GpuSet set(a.num("device", 0), 1, false);
    SketchSet ref, qry;
    string ref_path, qry_path;
    {   // .sketch inputs are read while the runtime starts
        string err;
        if (is_sketch_file(a.str("r", ""))) {
            ref_path = a.str("r", "");
            if (!read_sketches(ref_path, ref, err)) die("readSketches(), %s", err.c_str());
        }
        if (is_sketch_file(a.str("q", ""))) {
            qry_path = a.str("q", "");
            if (!read_sketches(qry_path, qry, err)) die("readSketches(), %s", err.c_str());
        }
    }
    if (ref_path.empty()) load_or_sketch(set[0], a.str("r", ""), a, threads, ref, ref_path);
    cerr << "the ref_sketch size is: " << ref.size() << endl;
    if (qry_path.empty()) load_or_sketch(set[0], a.str("q", ""), a, threads, qry, qry_path);
    if (qry.info.id != ref.info.id)
        die("command_lca(), the sketch infos between reference and query files are not match\n"
            "try to use the same shuffle file to generate sketches of the reference and query datasets");
    const size_t N = ref.size(), Q = qry.size();
    vector<uint32_t> taxa(N ? N : 1, RK_LCA_NONE);
    read_taxa(a.str("taxa", ""), N, tax, taxa);
    const bool missing = !exist_file(ref_path + ".index") || !exist_file(ref_path + ".dict");
    vector<rk_index *> idx(1, nullptr);
    build_everywhere(set, ref, ref_path, missing, idx);
    stamp("index built");
    if (getenv("RK_TIMING")) rk_ctx_set_timing(set[0].ctx, 1);
    const rk_lca_opts o{0, 0, 0};
    vector<uint64_t> off(Q + 1, 0);
    vector<uint32_t> matched(Q ? Q : 1, 0), unlabelled(Q ? Q : 1, 0), sizes(Q ? Q : 1, 0);
    for (size_t q = 0; q < Q; q++) sizes[q] = (uint32_t)(qry.off[q + 1] - qry.off[q]);
    rk_lca_count *counts = nullptr;
    uint64_t n_counts = 0;
    rk_lca_stats stats;
    rk_sketches *qs = upload(set[0], qry);
    set[0].check(rk_lca_rows(set[0].ctx, idx[0], qs, taxa.data(), tax.parent.data(), (uint32_t)tax.parent.size(), &o, off.data(), &counts, &n_counts, matched.data(),
                             unlabelled.data(), &stats), "rk_lca_rows");
    rk_sketches_free(qs);
    stamp("queries classified");
    vector<rk_lca_called> called(Q ? Q : 1);
    vector<uint32_t> clade(n_counts ? n_counts : 1, 0);
    if (rk_lca_call(counts, off.data(), (uint32_t)Q, sizes.data(), tax.parent.data(), (uint32_t)tax.parent.size(), &rule, called.data(), clade.data()) != 0)
        die("rk_lca_call failed");
    FILE *fp = fopen(a.str("o", "").c_str(), "w");
    if (!fp) die("cannot write %s", a.str("o", "").c_str());
    for (size_t q = 0; q < Q; q++) {
        const rk_lca_called &c = called[q];
        fprintf(fp, "%s\t", qry.names[q].c_str());
        if (c.taxon == RK_LCA_NONE) fprintf(fp, "-\t-\t");
        else fprintf(fp, "%llu\t%s\t", tax.id[c.taxon], tax.name[c.taxon].c_str());
        if (c.candidate == RK_LCA_NONE) fprintf(fp, "-");
        else fprintf(fp, "%llu", tax.id[c.candidate]);
        fprintf(fp, "\t%u\t%u\t%u\t%u\t%u\n", c.clade, c.retained, matched[q], unlabelled[q], sizes[q]);
    }
    fclose(fp);
    if (a.has("summary")) {
        FILE *sp = fopen(a.str("summary", "").c_str(), "w");
        if (!sp) die("cannot write %s", a.str("summary", "").c_str());
        for (size_t q = 0; q < Q; q++)
            for (uint64_t k = off[q]; k < off[q + 1]; k++)
                fprintf(sp, "%s\t%llu\t%s\t%u\t%u\n", qry.names[q].c_str(), tax.id[counts[k].taxon], tax.name[counts[k].taxon].c_str(), counts[k].direct, clade[k]);
        fclose(sp);
    }
    if (getenv("RK_TIMING"))
        fprintf(stderr, "[timing] %zu queries against %zu references under %zu nodes: %llu of %llu elements matched (%llu without a labelled holder), %llu records from "
                        "%llu partial records of %llu tiles, %llu lists (%llu by lane, %llu by wave, %llu by workgroup), longest climb %u, attempts %u, path %u, "
                        "%.3f ms on the device\n", Q, N, tax.parent.size(), (unsigned long long)stats.matched, (unsigned long long)stats.elements,
                (unsigned long long)stats.unlabelled, (unsigned long long)stats.records, (unsigned long long)stats.partials, (unsigned long long)stats.tiles,
                (unsigned long long)stats.lists, (unsigned long long)stats.lane_lists, (unsigned long long)stats.wave_lists, (unsigned long long)stats.block_lists,
                stats.longest_climb, stats.attempts, stats.path, rk_ctx_last_ms(set[0].ctx, RK_MS_LCA));
    rk_free_host(counts);
    rk_index_free(idx[0]);
    SelfJoin::leave();
}

// test helper: the text writer alone (no GPU): `_format alldist|dist names.txt hits.bin out pieces threads`;
// hits.bin = rk_hit records sorted by (row, col), dealt to `pieces` parts in blocks of 32 rows like --gpus does
static int cmd_format(int argc, char **argv)
{
    if (argc != 8) die("_format alldist|dist names.txt hits.bin out parts threads");
    const bool alldist = string(argv[2]) == "alldist";
    const vector<string> names = read_list(argv[3]);
    FILE *fp = fopen(argv[4], "rb");
    if (!fp) die("cannot open %s", argv[4]);
    vector<rk_hit> all;
    rk_hit h;
    while (fread(&h, sizeof(h), 1, fp) == 1) all.push_back(h);
    fclose(fp);
    const size_t G = (size_t)std::max(1, atoi(argv[6]));
    vector<vector<rk_hit>> per(G);
    for (const rk_hit &x : all) per[G == 1 ? 0 : (x.row / kRowBlock) % G].push_back(x);
    vector<HitPart> parts(G);
    for (size_t g = 0; g < G; g++) {
        parts[g].hits = per[g].data();
        parts[g].n = per[g].size();
        for (uint32_t r = 0; r < (uint32_t)names.size(); r++)
            if (G == 1 || (r / kRowBlock) % G == g) parts[g].rows.push_back(r);
    }
    write_hits(argv[5], parts, alldist, names, names, atoi(argv[7]));
    return 0;
}

static int cmd_info(const Args &a)
{
    if (!a.has("i")) die("info needs -i");
    SketchSet s;
    string err;
    if (!read_sketches(a.str("i", ""), s, err)) die("command_info(), %s", err.c_str());
    cerr << "the number of genome is: " << s.size() << endl;
    FILE *fp = fopen(a.str("o", "result.out").c_str(), "w+");
    if (!fp) die("cannot write %s", a.str("o", "result.out").c_str());
    fprintf(fp, "the number of sketches are: %d\n", (int)s.size());  // src/subCommand.cpp:93
    for (size_t i = 0; i < s.size(); i++) {
        const uint64_t cnt = s.off[i + 1] - s.off[i];
        fprintf(fp, "%s\t%d\n", s.names[i].c_str(), (int)cnt);
        if (a.has("F")) {
            for (uint64_t j = 0; j < cnt; j++) {
                if (s.wide()) fprintf(fp, "%lu\t", (unsigned long)s.hashes64[s.off[i] + j]);
                else fprintf(fp, "%u\t", s.hashes[s.off[i] + j]);
                if (j % 10 == 9) fprintf(fp, "\n");
            }
            fprintf(fp, "\n");
        }
    }
    fclose(fp);
    return 0;
}

// abund: what the side-car of a counted sketch (sketch --abund) holds.  Host only: no GPU is opened.
//   -i x.sketch [-o FILE] [--bins B]: per genome its name, distinct hashes, occurrences, largest count and lower median, then the
//   count spectrum (write_abund_report)
//   -i x.sketch --min-count N [--max-count M] -o y.sketch: the sketches reduced to the hashes with N <= count <= M, and y.sketch.abund
static int cmd_abund(const Args &a)
{
    if (!a.has("i")) die("abund needs -i");
    const string in = a.str("i", "");
    SketchSet s;
    string err;
    if (!read_sketches(in, s, err)) die("command_abund(), %s", err.c_str());
    if (!read_abund(abund_path(in), s, err)) die("command_abund(), %s", err.c_str());
    if (a.has("min-count") || a.has("max-count")) {
        const long long lo = atoll(a.str("min-count", "1").c_str()), hi = a.has("max-count") ? atoll(a.str("max-count", "").c_str()) : 0xFFFFFFFFLL;
        if (lo < 1) die("command_abund(), --min-count must be at least 1");
        if (hi < lo) die("command_abund(), --max-count must not be below --min-count");
        if (!a.has("o")) die("abund --min-count / --max-count needs -o");
        string out = a.str("o", "");
        if (!is_sketch_file(out)) out += ".sketch";
        SketchSet kept;
        abund_threshold(s, (uint32_t)std::min(lo, 0xFFFFFFFFLL), (uint32_t)std::min(hi, 0xFFFFFFFFLL), kept);
        if (!save_sketches(out, kept, err)) die("%s", err.c_str());
        if (!save_abund(abund_path(out), kept, err)) die("%s", err.c_str());
        cerr << "kept " << kept.total() << " of " << s.total() << " hashes of " << s.size() << " genomes" << endl;
        return 0;
    }
    const int bins = a.num("bins", 64);
    if (bins < 1) die("command_abund(), --bins must be at least 1");
    FILE *fp = a.has("o") ? fopen(a.str("o", "").c_str(), "w") : stdout;
    if (!fp) die("cannot write %s", a.str("o", "").c_str());
    write_abund_report(fp, s, (uint32_t)bins);
    if (fp != stdout) fclose(fp);
    return 0;
}

static int cmd_merge(const Args &a)
{
    if (!a.has("i") || !a.has("o")) die("merge needs -i and -o");
    SketchSet all;
    string err;
    bool first = true;
    for (const string &f : read_list(a.str("i", ""))) {
        if (!is_sketch_file(f)) die("command_merge(), the file: %s is not a sketch file in the list file: %s", f.c_str(), a.str("i", "").c_str());
        SketchSet s;
        if (!read_sketches(f, s, err)) die("command_merge(), %s", err.c_str());
        if (first) { all.info = s.info; first = false; }
        else if (s.info.id != all.info.id) die("command_merge(), mismatched sketch parameters in %s", f.c_str());
        const uint64_t b0 = all.total();
        all.names.insert(all.names.end(), s.names.begin(), s.names.end());
        all.hashes.insert(all.hashes.end(), s.hashes.begin(), s.hashes.end());
        all.hashes64.insert(all.hashes64.end(), s.hashes64.begin(), s.hashes64.end());
        for (size_t i = 1; i < s.off.size(); i++) all.off.push_back(b0 + s.off[i]);
    }
    string out = a.str("o", "");
    if (!is_sketch_file(out)) out += ".sketch";
    if (!save_sketches(out, all, err)) die("%s", err.c_str());
    return 0;
}

// ---- Kssd <-> RabbitKSSD conversion (src/sketch.cpp:1179-1365, src/subCommand.cpp:13-47) ------
struct CoDstat {  // co_dstat_t, src/sketch.h:38-47 (32 bytes, natural x86-64 layout)
    uint32_t shuf_id;
    uint8_t koc, pad_[3];
    int32_t kmerlen, dim_rd_len, comp_num, infile_num;
    uint64_t all_ctx_ct;
};
static_assert(sizeof(CoDstat) == 32, "co_dstat_t is 32 bytes");
static const int kPathLen = 256;  // PATHLEN, src/sketch.cpp:25

static int cmd_convert(const Args &a)
{
    if (!a.has("i") || !a.has("o")) die("convert needs -i and -o");
    const string in = a.str("i", ""), out_arg = a.str("o", "");
    string err;
    if (a.has("reverse")) {  // RabbitKSSD .sketch -> Kssd directory (:1288-1365)
        if (!is_sketch_file(in)) die("command_convert(), need input RabbitKSSD sketch file: %s", in.c_str());
        SketchSet s;
        if (!read_sketches(in, s, err)) die("readSketches(), %s", err.c_str());
        if (s.wide()) die("the Kssd sketch format holds 32-bit hashes only (half_k - drlevel <= 8)");
        if (mkdir(out_arg.c_str(), 0777) && errno != EEXIST) die("cannot create %s", out_arg.c_str());
        FILE *fs = fopen((out_arg + "/combco.0").c_str(), "w");
        if (!fs) die("cannot open: %s/combco.0", out_arg.c_str());
        fwrite(s.hashes.data(), 4, s.hashes.size(), fs);
        fclose(fs);
        FILE *fi = fopen((out_arg + "/combco.index.0").c_str(), "w+");
        if (!fi) die("cannot open: %s/combco.index.0", out_arg.c_str());
        fwrite(s.off.data(), 8, s.off.size(), fi);  // size_t prefix[infile_num+1]
        fclose(fi);
        CoDstat st{};
        st.shuf_id = (uint32_t)s.info.id;
        st.koc = 0;
        st.kmerlen = s.info.half_k * 2;
        st.dim_rd_len = s.info.drlevel * 2;
        st.comp_num = 1;
        st.infile_num = s.info.genomeNumber;
        st.all_ctx_ct = s.hashes.size();
        FILE *ft = fopen((out_arg + "/cofiles.stat").c_str(), "w+");
        if (!ft) die("cannot open: %s/cofiles.stat", out_arg.c_str());
        fwrite(&st, sizeof(st), 1, ft);
        for (size_t i = 0; i < s.size(); i++) {
            const uint32_t c = (uint32_t)(s.off[i + 1] - s.off[i]);
            fwrite(&c, 4, 1, ft);
        }
        for (size_t i = 0; i < s.size(); i++) {
            if (s.names[i].size() >= (size_t)kPathLen) die("genome name longer than %d bytes: %s", kPathLen - 1, s.names[i].c_str());
            char name[kPathLen] = {0};
            memcpy(name, s.names[i].data(), s.names[i].size());
            fwrite(name, 1, kPathLen, ft);
        }
        fclose(ft);
        return 0;
    }
    // Kssd directory -> .sketch (+ .dict/.index unless -q) (:1179-1285)
    FILE *ft = fopen((in + "/cofiles.stat").c_str(), "r");
    if (!ft) die("cannot open: %s/cofiles.stat", in.c_str());
    CoDstat st;
    if (fread(&st, sizeof(st), 1, ft) != 1 || st.infile_num < 0) die("convertSketch(), mismatched read cur_stat");
    SketchSet s;
    s.info.half_k = st.kmerlen / 2;
    s.info.half_subk = 6;  // hard-wired by the reference, :1197
    s.info.drlevel = st.dim_rd_len / 2;
    if (s.info.half_k - s.info.drlevel > 8) die("64-bit hash sketches are not supported by this build");
    const size_t n = (size_t)st.infile_num;
    vector<uint32_t> ctx_ct(n);
    if (fread(ctx_ct.data(), 4, n, ft) != n) die("convertSketch(), mismatched read tmp_ctx_ct");
    s.names.resize(n);
    for (size_t i = 0; i < n; i++) {
        char name[kPathLen + 1] = {0};
        if (fread(name, 1, kPathLen, ft) == 0) cerr << "Warning: convertSketch(), the read path length is zero " << endl;
        s.names[i] = name;
    }
    fclose(ft);
    FILE *fi = fopen((in + "/combco.index.0").c_str(), "rb");
    if (!fi) die("convertSketch(), cannot open: %s/combco.index.0", in.c_str());
    s.off.assign(n + 1, 0);
    if (fread(s.off.data(), 8, n + 1, fi) != n + 1) die("convertSketch(), mismatched read cbdcoindex");
    fclose(fi);
    FILE *fs = fopen((in + "/combco.0").c_str(), "rb");
    if (!fs) die("cannot open: %s/combco.0", in.c_str());
    s.hashes.resize(s.off[n]);
    if (st.all_ctx_ct != s.off[n] || fread(s.hashes.data(), 4, s.hashes.size(), fs) != s.hashes.size())
        die("the total hash number is not match to the state info, exit");
    fclose(fs);
    for (size_t i = 0; i < n; i++)
        if (s.off[i + 1] < s.off[i]) die("convertSketch(), corrupt combco.index.0");
    string out = out_arg;
    if (!is_sketch_file(out)) out += ".sketch";
    if (!save_sketches(out, s, err)) die("%s", err.c_str());
    if (!a.has("q")) {
        Gpu gpu(a.num("device", 0));
        rk_index_free(build_index(gpu, s, out, true));
    }
    return 0;
}

// ---- set algebra on sketch files (src/subCommand.cpp:307-794); host only ------------------
static int cmd_union(const Args &a)
{
    if (!a.has("i") || !a.has("o")) die("union needs -i and -o");
    const string in = a.str("i", "");
    if (!is_sketch_file(in)) die("command_union, %s is not sketch file, need input sketch file", in.c_str());
    SketchSet s;
    string err;
    if (!read_sketches(in, s, err)) die("command_union(), %s", err.c_str());
    cerr << "the total genome number in sketch file is: " << s.size() << endl;
    SketchSet u;
    u.info = s.info;
    // ascending hash order == the reference's bitmap walk (:493-520)
    if (s.wide()) {
        u.hashes64 = s.hashes64;
        std::sort(u.hashes64.begin(), u.hashes64.end());
        u.hashes64.erase(std::unique(u.hashes64.begin(), u.hashes64.end()), u.hashes64.end());
    } else {
        u.hashes = s.hashes;
        std::sort(u.hashes.begin(), u.hashes.end());
        u.hashes.erase(std::unique(u.hashes.begin(), u.hashes.end()), u.hashes.end());
    }
    u.names = {in + " merged sketches"};  // :372
    u.off = {0, s.wide() ? u.hashes64.size() : u.hashes.size()};
    if (!save_sketches(a.str("o", ""), u, err)) die("%s", err.c_str());
    return 0;
}

static int cmd_sub(const Args &a)
{
    if (!a.has("rs") || !a.has("qs") || !a.has("o")) die("sub needs --rs, --qs and -o");
    const string rs = a.str("rs", ""), qs = a.str("qs", "");
    if (!is_sketch_file(rs)) die("command_sub(), %s is not sketch file, need input sketch file", rs.c_str());
    if (!is_sketch_file(qs)) die("command_sub(): %s is not sketch file, need input sketch file", qs.c_str());
    SketchSet ref, qry;
    string err;
    if (!read_sketches(rs, ref, err)) die("command_sub(), %s", err.c_str());
    if (!read_sketches(qs, qry, err)) die("command_sub(), %s", err.c_str());
    if (qry.info.id != ref.info.id)
        die("command_sub(): the sketch infos between subtraction reference and query sketches are not same");
    SketchSet out;
    out.info = qry.info;
    out.names = qry.names;
    out.off.assign(1, 0);
    if (qry.wide()) {  // the reference's 2^bits bitmap (:561-572) is replaced by a sorted set
        vector<uint64_t> rs64 = ref.hashes64;
        std::sort(rs64.begin(), rs64.end());
        for (size_t i = 0; i < qry.size(); i++) {
            for (uint64_t e = qry.off[i]; e < qry.off[i + 1]; e++)
                if (!std::binary_search(rs64.begin(), rs64.end(), qry.hashes64[e])) out.hashes64.push_back(qry.hashes64[e]);
            out.off.push_back(out.hashes64.size());
        }
    } else {
        // one bit per hash value, MSB first (:575-583); sized by the sketches' hash space (2^28 values = 32 MiB of bits
        // at L3K10), not by the 2^32 of the type
        const int bits = std::min(32, std::max(1, 4 * (qry.info.half_k - qry.info.drlevel)));
        uint32_t top = 0;
        for (uint32_t h : ref.hashes) top = std::max(top, h);
        for (uint32_t h : qry.hashes) top = std::max(top, h);
        const uint64_t space = std::max<uint64_t>((uint64_t)1 << bits, (uint64_t)top + 1);  // a foreign file may exceed its declared space
        vector<uint64_t> dict((size_t)((space + 63) / 64), 0);
        for (uint32_t h : ref.hashes) dict[h / 64] |= 0x8000000000000000ULL >> (h % 64);
        for (size_t i = 0; i < qry.size(); i++) {
            for (uint64_t e = qry.off[i]; e < qry.off[i + 1]; e++) {
                const uint32_t h = qry.hashes[e];
                if (!(dict[h / 64] & (0x8000000000000000ULL >> (h % 64)))) out.hashes.push_back(h);
            }
            out.off.push_back(out.hashes.size());
        }
    }
    if (!save_sketches(a.str("o", ""), out, err)) die("%s", err.c_str());
    return 0;
}

// test helper: record reader parity (prints records, bases, FNV-1a hashes of the sequence and of the
// quality bytes, record end offsets -- the format of oracle/_ref/ref_driver kseq)
static int cmd_parse(int argc, char **argv)
{
    for (int i = 2; i < argc; i++) {
        vector<uint8_t> seq, qual;
        vector<uint64_t> off;
        if (!RecordReader::read_file(argv[i], seq, off, &qual)) die("cannot open %s", argv[i]);
        if (off.empty()) off.push_back(0);
        qual.resize(seq.size(), '~');
        {   // the packed sink must produce the same records, separated by 0x00
            vector<uint8_t> buf, packed;
            size_t n = 0;
            RecordReader::slurp(argv[i], buf, n);
            packed.assign(n + 2, 0xEE);
            const RecordReader::Packed pk = RecordReader::parse_packed(buf.data(), n, packed.data(), n + 1);
            vector<uint8_t> want;
            for (size_t r = 1; r < off.size(); r++) {
                want.insert(want.end(), seq.begin() + off[r - 1], seq.begin() + off[r]);
                if (r + 1 < off.size()) want.push_back(0);
            }
            if (pk.overflow || pk.n_rec != off.size() - 1 || pk.bytes != want.size() ||
                memcmp(want.data(), packed.data(), want.size()) != 0)
                die("packed parse differs from the vector parse for %s", argv[i]);
            // the parallel parser either declines or agrees
            for (int threads = 2; threads <= 5; threads += 3) {
                RecordReader::Packed pp;
                std::fill(packed.begin(), packed.end(), 0xEE);
                if (RecordReader::parse_packed_parallel(buf.data(), n, packed.data(), n + 1, threads, pp, 0) &&
                    (pp.overflow || pp.n_rec != pk.n_rec || pp.bytes != pk.bytes ||
                     memcmp(want.data(), packed.data(), want.size()) != 0))
                    die("parallel packed parse differs from the serial parse for %s (%d threads)", argv[i], threads);
            }
        }
        uint64_t h = 1469598103934665603ULL, hq = 1469598103934665603ULL;
        for (uint8_t c : seq) { h ^= c; h *= 1099511628211ULL; }
        for (uint8_t c : qual) { hq ^= c; hq *= 1099511628211ULL; }
        printf("%s\t%zu\t%zu\t%016llx\t%016llx", argv[i], off.size() - 1, seq.size(), (unsigned long long)h,
               (unsigned long long)hq);
        for (size_t r = 1; r < off.size(); r++) printf("\t%llu", (unsigned long long)off[r]);
        printf("\n");
    }
    return 0;
}

static int usage()
{
    cerr << "rabbit_kssd (MI355X build, " << rk_version() << ")\n"
            "subcommands: shuffle sketch abund alldist cluster forest greedy knn dbscan mreach medoid assign dist group union sub gather convert screen merge lca info mask\n"
            "  shuffle -k K -s S -l L -o out.shuf\n"
            "  sketch  -i genomes.list -o out[.sketch] [-L file.shuf] [-t T] [-q] [--abund] [--device N]   (--abund: also out.sketch.abund, how often every kept hash occurred in its genome or read set)\n"
            "  alldist -i in.sketch|genomes.list -o out [-D maxDist] [-M 0|1] [-L file.shuf] [--device N] [--gpus G]\n"
            "  cluster -i in.sketch|genomes.list -o out [-D maxDist] [-M 0|1] [-L file.shuf] [--device N] [--gpus G]   (single-linkage clusters of alldist's pairs)\n"
            "  forest -i in.sketch|genomes.list -o out [-D maxDist] [-M 0|1] [-L file.shuf] [--device N] [--gpus G]   (minimum spanning forest of alldist's pairs: the single-linkage dendrogram up to -D, one alldist line per edge)\n"
            "  greedy -i in.sketch|genomes.list -o out [-D maxDist] [-M 0|1] [--reps FILE] [-L file.shuf] [--device N]   (greedy representatives of alldist's pairs: larger sketch first, a genome joins the nearest earlier representative within -D or becomes one; one GPU)\n"
            "  knn -i in.sketch|genomes.list -o out -N k [-D maxDist] [-M 0|1] [-L file.shuf] [--device N] [--gpus G]   (the k nearest neighbours of every genome among alldist's pairs: one alldist-format line per genome and neighbour, nearest first)\n"
            "  dbscan -i in.sketch|genomes.list -o out -m minPts [-D maxDist] [-M 0|1] [-L file.shuf] [--device N]   (density-based clusters of alldist's pairs: a genome with minPts genomes, itself included, within -D is core; clusters are the components of the core genomes, a non-core genome joins its nearest core neighbour's cluster as border, the rest is noise; one GPU)\n"
            "  mreach -i in.sketch|genomes.list -o out -m minPts [-D maxDist] [-M 0|1] [--core FILE] [--cut t --labels FILE] [-L file.shuf] [--device N]   (minimum spanning forest of alldist's pairs under mutual-reachability distance, the HDBSCAN* hierarchy up to -D: one forest line per edge and its mutual-reachability distance; --core: every genome's core distance and the neighbour that sets it; --cut: the clusters of the core genomes at t <= maxDist, the rest as cluster 0; one GPU)\n"
            "  medoid -i in.sketch|genomes.list -o out [-D maxDist] [-M 0|1] [--by cluster|greedy|dbscan] [-m minPts] [--labels FILE] [--census FILE] [-L file.shuf] [--device N] [--gpus G]   (medoids and census of a clustering of alldist's pairs: per genome its cluster, its role -- the medoid is the member with the highest summed similarity to its fellow members --, its pairs inside the cluster and leaving it, its mean similarity to its fellow members and its nearest genome outside; the labels from --by (default cluster; dbscan needs -m; greedy and dbscan on one GPU) or from --labels: one line per genome, an integer below the number of genomes or -; --census: per cluster its size, medoid, inside pairs of size (size - 1) / 2, weakest inside pair and nearest leaving pair)\n"
            "  assign -r ref.sketch|list -q qry.sketch|list -D maxDist [-M 0|1] (--labels FILE | --by cluster|greedy|dbscan -m minPts) -o out [--novel FILE] [--gpus G] [--device N]   (placement of the queries into the clustered references: per query the cluster of its nearest labelled reference within -D, that reference's dist line, the query's references of that cluster, labelled and all within -D, and the runner-up cluster with its distance; - when novel; -D below 1.0; the labels from --labels -- one line per reference, an integer below their number or - -- or from --by on the same index (default cluster; dbscan needs -m and leaves non-core references unlabelled; greedy and dbscan on the first GPU); --novel: the names of the unplaced queries)\n"
            "  group -i in.sketch|genomes.list (--labels FILE | --by cluster|greedy|dbscan [-D 0.05] [-M 0|1] [-m 5]) [--pan | --core | --share P/Q] [--min-count C] [--only] -o out.sketch [--map FILE] [--device N]   (one sketch per cluster: --pan, the default, the union of its members' sketches; --core the hashes every member holds; --share P/Q those at least P of Q of its members hold; --min-count C: at least C members hold it; --only: no genome outside the cluster holds it -- its markers; the labels as medoid takes them; out.sketch: one sketch per cluster by ascending label, named after its first member; --map: per cluster its number, label, genomes, hashes kept and name; one GPU)\n"
            "  gather -r ref.sketch|list -q qry.sketch|list [--min-new 1] [--max-picks 0] [--sub host.sketch] -o out [--summary FILE] [--device N]   (which references explain each query, greedily: per round the reference that holds most of the query's hashes no earlier pick held, ties to the earlier reference, until a pick would add fewer than --min-new hashes or --max-picks are made; one line per pick: query, reference, rank, common|size_ref|size_query, fresh, fresh / size_query, common / size_ref; --summary: per query its name, size, hashes some reference holds, hashes the picks explain, references sharing at least --min-new hashes, picks; --sub: the queries first lose every hash a sketch of host.sketch holds, on the device -- the cover of what sub would write; one GPU)\n"
            "  screen  -r ref.sketch|list -q qry.sketch|list [--min-common 1] [--min-won 0] [--sub host.sketch] [--abund] -o out [--summary FILE] [--device N]   (which references are contained in each query, every shared hash credited to one of them -- mash screen -w in one pass: among the references that share at least --min-common hashes with the query a hash goes to the one with the larger common / size, compared exactly, then to the larger, then to the earlier one; one line per reference that keeps at least --min-won hashes: query, reference, common, size_ref, won, identity = (common / size_ref)^(1/K) and identity_won = (won / size_ref)^(1/K) for the sketches' k-mer length K; --summary: per query its name, size, hashes some reference holds, candidates, hashes claimed, records; --sub as in gather; --abund, for -q x.sketch with x.sketch.abund: four more columns, the lower median and the mean of the counts of the query's hashes over what the record shares, then over what it claims -- Mash's median multiplicity --, and three more in --summary: the sums of the counts over the whole sketch, its matched and its claimed hashes; the counts survive --sub; Mash's p-value is not offered; one GPU)\n"
            "  dist    -r ref.sketch|list -q qry.sketch|list -o out [-D maxDist] [-N n] [-M 0|1] [--device N] [--gpus G]\n"
            "  abund   -i in.sketch [-o out] [--bins 64]   |   abund -i in.sketch --min-count N [--max-count M] -o out.sketch   (the occurrence counts of a counted sketch, in.sketch.abund as sketch --abund writes it: per genome a line name, distinct hashes, occurrences, largest count, lower median, then count<TAB>hashes per non-empty bin below --bins and >=bins for the rest; with --min-count / --max-count the sketches reduced to the hashes whose count lies in [N, M], emptied genomes kept, and out.sketch.abund; host only)\n"
            "  info    -i in.sketch -o out [-F]\n"
            "  merge   -i sketches.list -o out.sketch\n"
            "  union   -i in.sketch -o out.sketch\n"
            "  sub     --rs ref.sketch --qs qry.sketch -o out.sketch\n"
            "  mask    -r ref.sketch|list -q qry.sketch|list [--keep absent|present | --min-refs A --max-refs B] [--abund] -o out.sketch [--device N]   (the query sketches with only the hashes that at least A and at most B reference sketches hold, hashes ascending: --keep absent, the default, is A = B = 0 -- the sketches sub writes, computed on the device; --keep present is A = 1 without B -- the intersection; --max-refs B alone drops the hashes more than B references hold, --min-refs A alone keeps those at least A hold; one GPU; --abund, for -q x.sketch with x.sketch.abund: every surviving hash keeps its count, in out.sketch.abund)\n"
            "  lca     -r ref.sketch|list -q qry.sketch|list --taxonomy FILE --taxa FILE [--min-count 1] [--confidence P/Q] [--of labelled|sketch] -o out [--summary FILE] [-L file.shuf] [--device N]   (every query classified by the lowest common ancestors of its hashes: a hash of the references carries the LCA of the taxa of the references that hold it, a query is the tally of those; --taxonomy: one line per node, id<TAB>parent id[<TAB>name], the root names itself; --taxa: one line per reference, an id of the taxonomy or -; the call is the LCA of the taxa with the highest root-to-node sum among those with at least --min-count hashes, moved towards the root until its clade holds P/Q of the hashes that carry a taxon, or with --of sketch of the whole sketch; one line per query: name, called id or -, its name, candidate id, clade, retained, matched, unlabelled, sketch size; --summary: per query and taxon its id, name, hashes and clade; one GPU)\n"
            "  convert -i kssd_dir -o out[.sketch] [-q]   |   convert --reverse -i in.sketch -o kssd_dir\n";
    return 1;
}

int main(int argc, char **argv)
{
    stamp("main");
    if (argc < 2) return usage();
    const string sub = argv[1];
    const std::map<string, string> alias = {
        {"-k", "k"}, {"--halfk", "k"}, {"-s", "s"}, {"--subk", "s"}, {"-l", "l"}, {"--reduction", "l"},
        {"-o", "o"}, {"--output", "o"}, {"-i", "i"}, {"--input", "i"}, {"-L", "L"}, {"-t", "t"}, {"--threads", "t"},
        {"-n", "n"}, {"--leastNumKmer", "n"}, {"-Q", "Q"}, {"--leastQuality", "Q"}, {"-D", "D"}, {"--maxDist", "D"},
        {"-M", "M"}, {"--metric", "M"}, {"-N", "N"}, {"--neighborN_max", "N"}, {"-r", "r"}, {"--reference", "r"},
        {"-F", "F"}, {"--Fined", "F"}, {"--device", "device"}, {"--query", "q"}, {"-q", "q"},
        {"--reverse", "reverse"}, {"--rs", "rs"}, {"--qs", "qs"}, {"--gpus", "gpus"}, {"--same-device", "same-device"}, {"--reps", "reps"}, {"-m", "m"}, {"--minPts", "m"}, {"--core", "core"}, {"--cut", "cut"}, {"--labels", "labels"}, {"--by", "by"}, {"--census", "census"}, {"--novel", "novel"},
        {"--pan", "pan"}, {"--share", "share"}, {"--min-count", "min-count"}, {"--only", "only"}, {"--map", "map"},
        {"--min-new", "min-new"}, {"--max-picks", "max-picks"}, {"--min-common", "min-common"}, {"--min-won", "min-won"}, {"--summary", "summary"}, {"--sub", "sub"},
        {"--keep", "keep"}, {"--min-refs", "min-refs"}, {"--max-refs", "max-refs"},
        {"--abund", "abund"}, {"--max-count", "max-count"}, {"--bins", "bins"},
        {"--taxonomy", "taxonomy"}, {"--taxa", "taxa"}, {"--confidence", "confidence"}, {"--of", "of"}};
    if (sub == "_parse") return cmd_parse(argc, argv);
    if (sub == "_format") return cmd_format(argc, argv);
    if (sub == "_layout") {  // test helper: the on-disk structs of this tool, in the format of `ref_driver layout`
        printf("sketchInfo_t %zu %zu %zu %zu %zu %zu\n", sizeof(SketchInfo), offsetof(SketchInfo, id), offsetof(SketchInfo, half_k),
               offsetof(SketchInfo, half_subk), offsetof(SketchInfo, drlevel), offsetof(SketchInfo, genomeNumber));
        printf("dim_shuffle_stat_t %zu %zu %zu %zu %zu\n", sizeof(ShufHeader), offsetof(ShufHeader, id), offsetof(ShufHeader, k),
               offsetof(ShufHeader, subk), offsetof(ShufHeader, drlevel));
        printf("co_dstat_t %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(CoDstat), offsetof(CoDstat, shuf_id), offsetof(CoDstat, koc),
               offsetof(CoDstat, kmerlen), offsetof(CoDstat, dim_rd_len), offsetof(CoDstat, comp_num), offsetof(CoDstat, infile_num),
               offsetof(CoDstat, all_ctx_ct));
        return 0;
    }
    if (sub == "shuffle") { cerr << "-----run the subcommand: shuffle" << endl; return cmd_shuffle(parse_args(argc, argv, 2, alias, {})); }
    // A distance run over .sketch files moves ~50 MB to the device and a few MB back, once: the runtime's DMA engines cost more to
    // set up (their queues: ~10 ms before the first upload, ~10 ms before the first read-back -- `index built` 34 -> 16 ms,
    // `distances` 14.6 -> 3.7 ms of the stamps of RK_TIMING) than blit kernels need to copy it.  Sketching from FASTA lists keeps
    // them: there gigabytes of uploads run beside the scan kernel.  (Set HSA_ENABLE_SDMA yourself to overrule.)
    if (sub == "alldist" || sub == "dist" || sub == "cluster" || sub == "forest" || sub == "greedy" || sub == "knn" || sub == "dbscan" || sub == "mreach" || sub == "medoid" || sub == "assign" || sub == "group" || sub == "gather" || sub == "mask" || sub == "lca" || sub == "screen") {
        bool from_sketches = true;
        for (int i = 2; i + 1 < argc; i++) {
            const string f = argv[i];
            if (f == "-i" || f == "--input" || f == "-r" || f == "--reference" || f == "-q" || f == "--query") from_sketches = from_sketches && is_sketch_file(argv[i + 1]);
        }
        if (from_sketches) setenv("HSA_ENABLE_SDMA", "0", 0);
    }
    // the GPU subcommands leave through _exit once their output is on disk (see Gpu::~Gpu)
    auto leave = [](int rc) -> int {
        stamp("done");
        fflush(stdout);
        fflush(stderr);
        _exit(rc);
        return rc;
    };
    if (sub == "sketch") { cerr << "-----run the subcommand: sketch" << endl; return leave(cmd_sketch(parse_args(argc, argv, 2, alias, {"q", "abund"}))); }
    if (sub == "alldist") { cerr << "-----run the subcommand: alldist" << endl; return leave(cmd_alldist(parse_args(argc, argv, 2, alias, {"same-device"}))); }
    if (sub == "cluster") { cerr << "-----run the subcommand: cluster" << endl; return leave(cmd_cluster(parse_args(argc, argv, 2, alias, {"same-device"}))); }
    if (sub == "forest") { cerr << "-----run the subcommand: forest" << endl; return leave(cmd_forest(parse_args(argc, argv, 2, alias, {"same-device"}))); }
    if (sub == "greedy") { cerr << "-----run the subcommand: greedy" << endl; return leave(cmd_greedy(parse_args(argc, argv, 2, alias, {"same-device"}))); }
    if (sub == "knn") { cerr << "-----run the subcommand: knn" << endl; return leave(cmd_knn(parse_args(argc, argv, 2, alias, {"same-device"}))); }
    if (sub == "dbscan") { cerr << "-----run the subcommand: dbscan" << endl; return leave(cmd_dbscan(parse_args(argc, argv, 2, alias, {"same-device"}))); }
    if (sub == "mreach") { cerr << "-----run the subcommand: mreach" << endl; return leave(cmd_mreach(parse_args(argc, argv, 2, alias, {"same-device"}))); }
    if (sub == "medoid") { cerr << "-----run the subcommand: medoid" << endl; return leave(cmd_medoid(parse_args(argc, argv, 2, alias, {"same-device"}))); }
    if (sub == "assign") { cerr << "-----run the subcommand: assign" << endl; return leave(cmd_assign(parse_args(argc, argv, 2, alias, {"same-device"}))); }
    if (sub == "group") { cerr << "-----run the subcommand: group" << endl; return leave(cmd_group(parse_args(argc, argv, 2, alias, {"pan", "core", "only"}))); }   // (--core is a flag here, a file of mreach)
    if (sub == "gather") { cerr << "-----run the subcommand: gather" << endl; return leave(cmd_gather(parse_args(argc, argv, 2, alias, {}))); }
    if (sub == "screen") { cerr << "-----run the subcommand: screen" << endl; return leave(cmd_screen(parse_args(argc, argv, 2, alias, {"abund"}))); }
    if (sub == "mask") { cerr << "-----run the subcommand: mask" << endl; return leave(cmd_mask(parse_args(argc, argv, 2, alias, {"abund"}))); }
    if (sub == "lca") { cerr << "-----run the subcommand: lca" << endl; return leave(cmd_lca(parse_args(argc, argv, 2, alias, {}))); }
    if (sub == "dist") { cerr << "-----run the subcommand: dist" << endl; return leave(cmd_dist(parse_args(argc, argv, 2, alias, {"same-device"}))); }
    if (sub == "abund") { cerr << "-----run the subcommand: abund" << endl; return cmd_abund(parse_args(argc, argv, 2, alias, {})); }
    if (sub == "info") { cerr << "-----run the subcommand: info" << endl; return cmd_info(parse_args(argc, argv, 2, alias, {"F"})); }
    if (sub == "merge") { cerr << "-----run the subcommand: merge" << endl; return cmd_merge(parse_args(argc, argv, 2, alias, {})); }
    if (sub == "convert") { cerr << "-----run the subcommand: convert" << endl; return cmd_convert(parse_args(argc, argv, 2, alias, {"q", "reverse"})); }
    if (sub == "union") { cerr << "-----run the subcommand: union" << endl; return cmd_union(parse_args(argc, argv, 2, alias, {})); }
    if (sub == "sub") { cerr << "-----run the subcommand: sub" << endl; return cmd_sub(parse_args(argc, argv, 2, alias, {})); }
    return usage();
}
