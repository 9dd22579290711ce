// sketch_input.hpp -- what `rabbit_kssd sketch` does to its input files in front of the GPU, host-only: the batch plan
// of a file list, and the two streamed readers of one big file (the role of src/sketch.cpp:380-450 and :658-737: RabbitFX
// chunks of a big file go to the consumers while the producer is still reading).  A reader turns a file into the packed
// layout rk_sketch_packed_dev expects (records separated by 0x00, zero padding: invalid bases) piece by piece and hands
// the pieces to an InputSink: page-locked buffers, uploads and a device buffer in rabbit_kssd.cpp, plain memory in
// tools/sketch_input_check.cpp.  A piece starts with the last k-1 bases in front of it unless a header line lies between,
// so that every window is seen exactly once -- by the piece it ENDS in --, and a zero byte follows every piece.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <utility>

#include "formats.hpp"

namespace rkhost {

// ---- the sink: all a streamed reader needs of a GPU (every call comes from the thread that called the reader) ------
struct InputSink {
    virtual ~InputSink() {}
    virtual uint8_t *ring_alloc(uint64_t bytes) = 0;                          // one buffer of the ring (page-locked)
    virtual void ring_free(uint8_t *p) = 0;
    virtual void grow(uint64_t cap, uint64_t used) = 0;                       // a (device) buffer of `cap` bytes that keeps the first `used`
    virtual void put(uint64_t off, const uint8_t *src, uint64_t bytes) = 0;   // returns when the bytes are there: src is free again
    virtual void complete(uint64_t used) = 0;                                 // the buffer holds the whole file in [0, used)
};

struct StreamStats {   // for the [timing] lines of the tool
    size_t pieces = 0;
    int ring = 0, parsers = 0;
    uint64_t slot_bytes = 0, dev_bytes = 0, text_bytes = 0, used = 0;
    double alloc_sec = 0, stream_sec = 0;   // up to the last allocation / up to the last put, both from the call
};

inline double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// piece size of a streamed big file: RK_BIG_PIECE_MB (default 32), RK_BIG_PIECE_KB (tests) wins; at least 1 of its unit
inline size_t big_piece_bytes()
{
    size_t piece = (size_t)(getenv("RK_BIG_PIECE_MB") ? std::max(1, atoi(getenv("RK_BIG_PIECE_MB"))) : 32) << 20;
    if (getenv("RK_BIG_PIECE_KB")) piece = (size_t)std::max(1, atoi(getenv("RK_BIG_PIECE_KB"))) << 10;
    return piece;
}
// initial device capacity of the sequential reader: at least 256 MiB; RK_BIG_DEV_MB (tests: force the growth) wins
inline uint64_t sequential_dev_cap(const std::string &path)
{
    struct stat st;
    uint64_t dev_cap = 256ull << 20;
    if (stat(path.c_str(), &st) == 0) dev_cap = std::max<uint64_t>(dev_cap, (uint64_t)st.st_size * (ends_with(path, ".gz") ? 4 : 1) + (64ull << 20));
    if (getenv("RK_BIG_DEV_MB")) dev_cap = (uint64_t)std::max(1, atoi(getenv("RK_BIG_DEV_MB"))) << 20;
    return dev_cap;
}

// ---- cut rules -----------------------------------------------------------------------------------------------------
// a mapped file: a cut at the next line start at or after `piece` bytes behind the cut before; cuts.front() == 0, cuts.back() == sz
inline std::vector<size_t> mapped_cuts(const uint8_t *b, size_t sz, size_t piece)
{
    std::vector<size_t> cut{0};
    while (cut.back() < sz) {
        size_t p = std::min(sz, cut.back() + piece);
        if (p < sz) {
            const void *e = memchr(b + p, '\n', sz - p);
            p = e ? (size_t)((const uint8_t *)e - b) + 1 : sz;
        }
        cut.push_back(p);
    }
    return cut;
}

// Where a text that was read sequentially may be cut so that what follows parses on its own: the length of the part to
// keep, 0 when there is no such place.  FASTA: behind the last newline.
inline size_t fasta_cut_point(const uint8_t *b, size_t n)
{
    const void *q = memrchr(b, '\n', n);
    return q ? (size_t)((const uint8_t *)q - b) + 1 : 0;
}
// FASTQ: the last '@' line start whose next line but one starts with '+' (a quality line may start with '@' too: the
// line after ITS next is a sequence line, never '+')
inline size_t fastq_cut_point(const uint8_t *b, size_t n)
{
    size_t pos = n;
    for (int tries = 0; tries < 4096 && pos > 0; tries++) {
        const void *q = memrchr(b, '\n', pos - 1);
        const size_t ls = q ? (size_t)((const uint8_t *)q - b) + 1 : 0;
        if (b[ls] == '@') {
            const void *e1 = memchr(b + ls, '\n', n - ls);
            const void *e2 = e1 ? memchr((const uint8_t *)e1 + 1, '\n', n - ((const uint8_t *)e1 + 1 - b)) : nullptr;
            if (e2 && (size_t)((const uint8_t *)e2 + 1 - b) < n && ((const uint8_t *)e2)[1] == '+') {
                // ... and, so that a quality line that starts with '@' inside a MULTI-line record (two lines further on: another
                // quality line starting with '+': both are valid Phred characters) is not taken for a record start: the
                // candidate's sequence line and its quality line have the same length (a four-line record; a multi-line file
                // offers no such candidate and takes the whole-file path)
                const uint8_t *p3 = (const uint8_t *)e2 + 1;
                const void *e3 = memchr(p3, '\n', n - (size_t)(p3 - b));
                const uint8_t *p4 = e3 ? (const uint8_t *)e3 + 1 : nullptr;
                const void *e4 = p4 ? memchr(p4, '\n', n - (size_t)(p4 - b)) : nullptr;
                if (e4) {
                    auto len = [](const uint8_t *a, const void *e) { size_t l = (size_t)((const uint8_t *)e - a); return l && a[l - 1] == '\r' ? l - 1 : l; };
                    if (len((const uint8_t *)e1 + 1, e2) == len(p4, e4)) return ls;
                }
            }
        }
        if (ls == 0) break;
        pos = ls;   // (the newline before this line start is at ls - 1)
        if (pos == 0) break;
    }
    return 0;
}

// ---- the backward walk ---------------------------------------------------------------------------------------------
// FASTA: the last `need` (<= 63) bases in front of t[n], a line start, unless a header line lies between: walked
// backwards line by line.  Where the walk reaches t[0] without a header line and is still short, it goes on in `older`:
// the bases in front of t, no line structure (the mapped file has none: t is the file).  Writes the bases to
// out[0, returned).  (A '+' or '@' line counts as bases here: the line walk of the piece that holds it refuses the file.)
inline size_t bases_before(const uint8_t *t, size_t n, const uint8_t *older, size_t n_older, size_t need, uint8_t *out)
{
    uint8_t tmp[64];
    size_t got = 0;
    size_t le = n;   // one past the newline that ends the line being looked at
    while (got < need && le > 0) {
        const size_t nl = le - 1;   // t[nl] == '\n'
        const void *q = nl ? memrchr(t, '\n', nl) : nullptr;
        const size_t ls = q ? (size_t)((const uint8_t *)q - t) + 1 : 0;
        if (t[ls] == '>') { n_older = 0; break; }   // a record starts here: nothing in front of it belongs to the windows behind
        for (size_t c = nl; c > ls && got < need; c--) tmp[need - 1 - got++] = t[c - 1];
        le = ls;
    }
    for (size_t c = n_older; c > 0 && got < need; c--) tmp[need - 1 - got++] = older[c - 1];
    memcpy(out, tmp + (need - got), got);
    return got;
}

// ---- the ring ------------------------------------------------------------------------------------------------------
// `slots` numbered buffers (or tokens) between producers and one consumer: a producer acquires a free slot, fills it and
// publishes it with a payload; the consumer takes (payload, slot) in the order of publication and releases the slot.
// take() returns false once every producer has said producer_done() and nothing is left.
template <class Payload> class PieceRing {
  public:
    PieceRing(int slots, int producers) : producers_(producers)
    {
        for (int j = 0; j < slots; j++) free_.push_back(j);
    }
    int acquire()
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !free_.empty(); });
        const int j = free_.front();
        free_.pop_front();
        return j;
    }
    void publish(Payload p, int slot)
    {
        { std::lock_guard<std::mutex> lk(mu_); ready_.emplace_back(std::move(p), slot); }
        cv_.notify_all();
    }
    void producer_done()
    {
        { std::lock_guard<std::mutex> lk(mu_); producers_--; }
        cv_.notify_all();
    }
    bool take(Payload &p, int &slot)
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !ready_.empty() || producers_ == 0; });
        if (ready_.empty()) return false;
        p = std::move(ready_.front().first);
        slot = ready_.front().second;
        ready_.pop_front();
        return true;
    }
    void release(int slot)
    {
        { std::lock_guard<std::mutex> lk(mu_); free_.push_back(slot); }
        cv_.notify_all();
    }

  private:
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<int> free_;
    std::deque<std::pair<Payload, int>> ready_;
    int producers_;
};

// ---- one big plain FASTA file, mapped and cut at line starts ---------------------------------------------------------
// Parser threads turn piece after piece into the packed layout -- ONE pass, straight into a small ring of buffers -- and
// the calling thread puts every finished piece into its own slot of the sink's buffer.  Slots are sized for the piece's
// file bytes (newlines become padding), so no piece has to know how much the pieces before it shrank.
// Returns false -- complete() was not called -- for inputs this path does not take (under 64 bytes, no '>' at the start,
// '+' / '@' lines, '\r' line ends): the caller falls back to the whole-file path.
inline bool stream_mapped_fasta(const std::string &path, int kmer, int threads, size_t piece, InputSink &sink, StreamStats &st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct stat fst;
    if (fstat(fd, &fst) || fst.st_size < 64) { close(fd); return false; }
    const size_t sz = (size_t)fst.st_size;
    const uint8_t *b = (const uint8_t *)mmap(nullptr, sz, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (b == MAP_FAILED) return false;
    (void)madvise((void *)b, sz, MADV_SEQUENTIAL);
    struct Unmap { const uint8_t *p; size_t n; ~Unmap() { munmap((void *)p, n); } } unmap{b, sz};
    if (b[0] != '>') return false;   // (kseq skips to the first header: leave odd files to the serial reader)

    const std::vector<size_t> cut = mapped_cuts(b, sz, piece);
    const size_t n_pieces = cut.size() - 1;
    std::vector<uint64_t> slot_off(n_pieces + 1, 0);
    uint64_t max_slot = 0;
    for (size_t i = 0; i < n_pieces; i++) {
        const uint64_t cap = ((cut[i + 1] - cut[i]) + (uint64_t)kmer + 2 + 1023) & ~1023ULL;   // prefix + separator + the piece
        slot_off[i + 1] = slot_off[i] + cap;
        max_slot = std::max(max_slot, cap);
    }
    const uint64_t dev_bytes = slot_off[n_pieces];
    const int n_ring = (int)std::min<size_t>(n_pieces, (size_t)std::max(2, std::min(threads, 8)));
    const int nt = (int)std::min<size_t>(n_pieces, (size_t)std::max(1, threads));
    sink.grow(dev_bytes, 0);
    std::vector<uint8_t *> slots((size_t)n_ring, nullptr);
    for (auto &s : slots) s = sink.ring_alloc(max_slot);
    st.pieces = n_pieces, st.ring = n_ring, st.parsers = nt;
    st.slot_bytes = max_slot, st.dev_bytes = st.used = dev_bytes, st.text_bytes = sz;
    st.alloc_sec = seconds_since(t0);

    PieceRing<size_t> ring(n_ring, nt);
    std::atomic<size_t> next_piece{0};
    std::atomic<bool> bad{false};
    const size_t need = (size_t)std::min(63, kmer - 1);
    auto parse_piece = [&](size_t i, uint8_t *dst) {
        uint8_t *w = dst;
        if (i > 0) w += bases_before(b, cut[i], nullptr, 0, need, w);
        const RecordReader::Lines r = RecordReader::walk_fasta_lines(b + cut[i], cut[i + 1] - cut[i], i == 0, w);
        if (r.bad) { bad = true; return; }
        w += r.bytes;
        memset(w, 0, (size_t)(dst + (slot_off[i + 1] - slot_off[i]) - w));   // padding: invalid bases
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; t++)
        pool.emplace_back([&]() {
            for (;;) {
                const size_t i = next_piece.fetch_add(1);
                if (i >= n_pieces) break;
                const int j = ring.acquire();
                if (!bad) parse_piece(i, slots[(size_t)j]);
                ring.publish(i, j);
            }
            ring.producer_done();
        });
    // this thread: every finished piece to its slot of the sink's buffer, while the others are parsed
    size_t i = 0;
    int j = 0;
    while (ring.take(i, j)) {
        if (!bad) sink.put(slot_off[i], slots[(size_t)j], slot_off[i + 1] - slot_off[i]);
        ring.release(j);
    }
    for (auto &th : pool) th.join();
    st.stream_sec = seconds_since(t0);
    const bool ok = !bad;
    if (ok) sink.complete(dev_bytes);
    for (uint8_t *s : slots) sink.ring_free(s);
    return ok;
}

// ---- one big gzip'ed file, or one big FASTQ file, read sequentially ------------------------------------------------
// A reader thread (gzread: plain, gzip'ed and multi-member files alike) fills text pieces of `piece` bytes, each cut
// where the parser of a piece needs no context: a FASTQ piece ends in front of a record (RecordReader::parse_packed --
// kseq semantics, quality gate -- parses it like a file of its own), a FASTA piece at a line start and carries the bases
// in front of it.  Parser threads turn pieces into the packed layout in a ring of buffers, the calling thread puts them
// into consecutive stretches of the sink's buffer, which doubles when the inflated size outgrows it, and complete() sees
// the whole file (so -n, the minimum number of occurrences, counts over the whole file).
// Returns false -- complete() was not called -- for inputs this path does not take ('\r' line ends or '+' / '@' lines in
// FASTA, no cut point inside a piece, a FASTQ piece that overflows its slot, no header at the start).
inline bool stream_sequential(const std::string &path, bool fastq, int least_qual, int kmer, int threads, size_t piece, uint64_t dev_cap,
                              InputSink &sink, StreamStats &st)
{
    const auto t0 = std::chrono::steady_clock::now();
    gzFile fp = gzopen(path.c_str(), "r");
    if (!fp) return false;
    gzbuffer(fp, 1 << 20);
    const size_t need = (size_t)std::min(63, kmer - 1);
    struct Piece {
        RawBuf text;
        size_t len = 0;
        uint8_t prefix[64];
        size_t n_prefix = 0;
        bool first = false;
        uint64_t cap = 0;   // packed bytes, padded to 1 KiB
    };
    typedef std::unique_ptr<Piece> PiecePtr;
    const int n_ring = std::max(2, std::min(threads, 4));
    const int nt = std::max(1, std::min(threads, n_ring));
    const uint64_t slot_cap = ((uint64_t)piece * 2 + (uint64_t)kmer + 2 + 1024 + 1023) & ~1023ULL;   // (a piece holds at most 2 x `piece` text bytes)
    std::vector<uint8_t *> slots((size_t)n_ring, nullptr);
    for (auto &s : slots) s = sink.ring_alloc(slot_cap);
    dev_cap = (dev_cap + 1023) & ~1023ULL;
    sink.grow(dev_cap, 0);
    st.alloc_sec = seconds_since(t0);

    PieceRing<PiecePtr> texts(n_ring, 1);   // read, not yet parsed (the slots are tokens: the reader runs at most n_ring pieces ahead)
    PieceRing<PiecePtr> ring(n_ring, nt);   // parsed into a ring buffer
    std::atomic<bool> bad{false};

    std::thread reader([&]() {
        PiecePtr cur(new Piece);
        cur->text.resize(2 * piece + (1u << 20));
        cur->first = true;
        uint8_t carry_prefix[64];
        size_t n_carry_prefix = 0;
        for (;;) {
            // fill the current piece up to `piece` bytes beyond what it already holds
            bool end = false;
            while (cur->len < piece) {
                const int r = gzread(fp, cur->text.data() + cur->len, (unsigned)std::min<size_t>(piece - cur->len, 1u << 30));
                if (r <= 0) { end = true; break; }
                cur->len += (size_t)r;
            }
            if (cur->first && cur->len && cur->text.data()[0] != (fastq ? '@' : '>')) { bad = true; end = true; cur->len = 0; }
            PiecePtr next(new Piece);
            if (!end) {
                const size_t keep = fastq ? fastq_cut_point(cur->text.data(), cur->len) : fasta_cut_point(cur->text.data(), cur->len);
                if (keep == 0) { bad = true; end = true; cur->len = 0; }   // no cut point inside a piece: not a file for this path
                else {
                    next->text.resize(2 * piece + (1u << 20));
                    next->len = cur->len - keep;
                    memcpy(next->text.data(), cur->text.data() + keep, next->len);
                    cur->len = keep;
                }
            }
            if (!fastq && cur->len) {
                memcpy(cur->prefix, carry_prefix, n_carry_prefix);
                cur->n_prefix = cur->first ? 0 : n_carry_prefix;
                // (a piece with fewer than k-1 bases of its own hands the bases in front of it on)
                n_carry_prefix = bases_before(cur->text.data(), cur->len, cur->prefix, cur->n_prefix, need, carry_prefix);
            }
            if (cur->len) {
                const int token = texts.acquire();
                st.text_bytes += cur->len;   // (this thread alone, read after its join)
                st.pieces++;
                texts.publish(std::move(cur), token);
            }
            if (end) break;
            cur = std::move(next);
        }
        texts.producer_done();
    });

    auto parse_piece = [&](Piece &pc, uint8_t *dst) -> uint64_t {   // returns the bytes written (padded to 1 KiB by the caller)
        uint8_t *w = dst;
        const uint8_t *b = pc.text.data();
        if (fastq) {
            const RecordReader::Packed pk = RecordReader::parse_packed(b, pc.len, w, slot_cap - 1024, least_qual);
            if (pk.overflow) { bad = true; return 0; }
            w += pk.bytes;
        } else {
            memcpy(w, pc.prefix, pc.n_prefix);
            w += pc.n_prefix;
            const RecordReader::Lines r = RecordReader::walk_fasta_lines(b, pc.len, pc.first, w);
            if (r.bad) { bad = true; return 0; }
            w += r.bytes;
        }
        *w++ = 0;   // whatever follows in the buffer starts a new record (a piece of a multiple of 1 KiB gets no padding)
        return (uint64_t)(w - dst);
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; t++)
        pool.emplace_back([&]() {
            PiecePtr pc;
            int token = 0;
            while (texts.take(pc, token)) {
                texts.release(token);
                const int j = ring.acquire();
                const uint64_t bytes = bad ? 0 : parse_piece(*pc, slots[(size_t)j]);
                pc->cap = (bytes + 1023) & ~1023ULL;
                memset(slots[(size_t)j] + bytes, 0, (size_t)(pc->cap - bytes));   // padding: invalid bases
                ring.publish(std::move(pc), j);
            }
            ring.producer_done();
        });
    // this thread: every parsed piece to the next free stretch of the sink's buffer
    uint64_t dev_used = 0;
    PiecePtr pc;
    int j = 0;
    while (ring.take(pc, j)) {
        if (!bad && pc->cap) {
            if (dev_used + pc->cap > dev_cap) {   // the inflated file outgrew the buffer: twice the size, copy, go on
                dev_cap = std::max(dev_cap * 2, dev_used + pc->cap);
                sink.grow(dev_cap, dev_used);
            }
            sink.put(dev_used, slots[(size_t)j], pc->cap);
            dev_used += pc->cap;
        }
        ring.release(j);
    }
    reader.join();
    for (auto &th : pool) th.join();
    gzclose(fp);
    st.ring = n_ring, st.parsers = nt, st.slot_bytes = slot_cap, st.dev_bytes = dev_cap, st.used = dev_used;
    st.stream_sec = seconds_since(t0);
    const bool ok = !bad;
    if (ok) sink.complete(dev_used);
    for (uint8_t *s : slots) sink.ring_free(s);
    return ok;
}

// ---- the batch plan of a file list: batches that fit one staging buffer, every file in a 1 KiB-aligned slot ----------
struct Slot {
    uint64_t off = 0, cap = 0;  // position / capacity in the staging buffer
    uint64_t len = 0;           // packed bytes written
    bool overflow = false;      // the size estimate was too small (multi-member .gz): slow path
};
struct Batch {
    size_t first = 0, last = 0;  // files [first, last)
    uint64_t bytes = 0;          // staging bytes used
    bool pageable = false;       // one oversized file: staged in ordinary memory
    bool streamed = false;       // ... or streamed piece by piece (stream_mapped_fasta / stream_sequential)
    std::vector<Slot> slots;
};

// upper bound of a file's packed size: a plain file cannot expand; a .gz member stores its length mod 2^32 in the
// trailer (the last member's: a multi-member file may overflow its slot).  false: the file cannot be opened
inline bool packed_bound(const std::string &f, uint64_t &bound)
{
    struct stat st;
    if (stat(f.c_str(), &st)) return false;
    uint64_t sz = (uint64_t)st.st_size;
    FILE *fp = fopen(f.c_str(), "rb");
    if (!fp) return false;
    unsigned char m[2] = {0, 0}, tail[4];
    if (fread(m, 1, 2, fp) == 2 && m[0] == 0x1f && m[1] == 0x8b && sz >= 18 && !fseek(fp, -4, SEEK_END) &&
        fread(tail, 1, 4, fp) == 4) {
        const uint64_t isize = (uint64_t)tail[0] | ((uint64_t)tail[1] << 8) | ((uint64_t)tail[2] << 16) |
                               ((uint64_t)tail[3] << 24);
        sz = std::max<uint64_t>(isize, sz);
    }
    fclose(fp);
    bound = sz;
    return true;
}
// the slot of a file: its packed bytes, the separator behind them, 1 KiB-aligned
inline uint64_t slot_bound(uint64_t packed) { return (packed + 1 + 1023) & ~1023ULL; }

// staging buffers: two, an eighth of the input each (uploads and kernels overlap the parsing of the next batch), between
// 64 and 256 MiB -- page-locking costs 0.2 s per GB and releasing 0.13 s per GB (measured: 2 x 1 GiB for 1,000 x 5 Mb
// were 0.42 + 0.27 s of a 1.4 s run whose parsing, uploads and kernels take 0.2 s).  RK_STAGE_MB wins.
inline uint64_t stage_size(uint64_t total_bound)
{
    uint64_t stage_bytes = std::min<uint64_t>(256ull << 20, std::max<uint64_t>(64ull << 20, total_bound / 8));
    if (getenv("RK_STAGE_MB")) stage_bytes = std::max<uint64_t>(1, (uint64_t)atoll(getenv("RK_STAGE_MB"))) << 20;
    return (stage_bytes + 1023) & ~1023ULL;
}

// a file bigger than the staging buffer: alone, pageable (page-locking and releasing 3 GB costs 0.9 s, the slower upload 0.2 s)
inline std::vector<Batch> plan_batches(const std::vector<uint64_t> &bound, uint64_t stage_bytes)
{
    std::vector<Batch> batches;
    for (size_t i = 0; i < bound.size();) {
        Batch bt;
        bt.first = i;
        bt.pageable = bound[i] > stage_bytes;
        do {   // the first file always, further ones while they fit
            Slot sl;
            sl.off = bt.bytes;
            sl.cap = bound[i];
            bt.slots.push_back(sl);
            bt.bytes += bound[i++];
        } while (!bt.pageable && i < bound.size() && bt.bytes + bound[i] <= stage_bytes);
        bt.last = i;
        batches.push_back(std::move(bt));
    }
    return batches;
}

}  // namespace rkhost
