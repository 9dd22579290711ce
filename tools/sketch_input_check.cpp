// Developer check: host/sketch_input.hpp as a stand-alone program (plain C++, no HIP, no GPU).  It runs the streamed readers of
// `rabbit_kssd sketch` with a sink of plain memory and prints, per case, what tests/test_sketch_input_cpu.py compares: whether
// the reader declined, the digest of the multiset of k-byte windows without a 0x00 byte in the sink's buffer [0, used) and in
// RecordReader::parse_packed of the whole text ("every window is seen exactly once"), and what the sink saw of the rules of a put;
// and the batch plan of a list for given slot bounds.  Cases come from a file, one per line:
//   mapped <file> <k> <piece bytes> <threads>
//   seq <file> fa|fq <least_qual> <k> <piece bytes> <threads> <initial capacity>
//   plan <bound> ...          (RK_STAGE_MB from the environment)
//   bound <file>
//   g++ -O1 -g -std=c++17 -Wall -Werror [-fsanitize=thread | -fsanitize=address,undefined] -Irabbitkssd_amd/host tools/sketch_input_check.cpp
//       -o sketch_input_check -lz -lpthread && ./sketch_input_check cases.txt
#include <cinttypes>
#include <sstream>

#include "sketch_input.hpp"

using namespace rkhost;

static const uint8_t POISON = 0xEE;   // no base, no separator, no padding: memory that nobody wrote

struct HostSink : InputSink {
    std::vector<uint8_t> buf;
    uint64_t used = 0;
    int completed = 0, grows = 0, puts = 0;
    // what must never happen: a put that is not 1 KiB-aligned in offset or length / beyond the capacity of the last grow / a grow
    // that would drop what was put
    int unaligned = 0, beyond = 0, shrunk = 0;
    uint8_t *ring_alloc(uint64_t bytes) override
    {
        uint8_t *p = (uint8_t *)malloc(bytes);
        memset(p, POISON, bytes);
        return p;
    }
    void ring_free(uint8_t *p) override { free(p); }
    void grow(uint64_t cap, uint64_t keep) override
    {
        grows++;
        if (keep > buf.size() || cap < keep) { shrunk++; return; }
        std::vector<uint8_t> bigger(cap, POISON);
        if (keep) memcpy(bigger.data(), buf.data(), keep);
        buf.swap(bigger);
    }
    void put(uint64_t off, const uint8_t *src, uint64_t bytes) override
    {
        puts++;
        if ((off & 1023) || (bytes & 1023)) unaligned++;
        if (off + bytes > buf.size()) { beyond++; return; }
        memcpy(buf.data() + off, src, bytes);
        memset(const_cast<uint8_t *>(src), POISON, bytes);   // the ring buffer is free again: what its next user does not write shows
    }
    void complete(uint64_t n) override { used = n; completed++; }
};

struct Digest {   // of a multiset of windows: their number, the sum and the xor of their FNV-1a hashes
    uint64_t n = 0, sum = 0, x = 0;
};
static Digest windows(const uint8_t *b, size_t n, size_t k)
{
    Digest d;
    size_t run = 0;   // bytes since the last 0x00
    for (size_t i = 0; i < n; i++) {
        run = b[i] ? run + 1 : 0;
        if (run < k) continue;
        uint64_t h = 1469598103934665603ULL;
        for (size_t j = i + 1 - k; j <= i; j++) { h ^= b[j]; h *= 1099511628211ULL; }
        d.n++;
        d.sum += h;
        d.x ^= h;
    }
    return d;
}

static void streamed_case(const std::string &line, bool mapped, std::istringstream &in)
{
    std::string path, kind = "fa";
    int least_qual = 0, k = 0, threads = 1;
    size_t piece = 0;
    uint64_t cap = 0;
    in >> path;
    if (!mapped) in >> kind >> least_qual;
    in >> k >> piece >> threads;
    if (!mapped) in >> cap;
    HostSink sink;
    StreamStats st;
    const bool ok = mapped ? stream_mapped_fasta(path, k, threads, piece, sink, st)
                           : stream_sequential(path, kind == "fq", least_qual, k, threads, piece, cap, sink, st);
    if (!ok) {
        printf("%s : declined completed=%d\n", line.c_str(), sink.completed);
        return;
    }
    uint64_t poison = 0;
    for (uint64_t i = 0; i < sink.used && i < sink.buf.size(); i++) poison += sink.buf[i] == POISON;
    const Digest got = windows(sink.buf.data(), (size_t)std::min<uint64_t>(sink.used, sink.buf.size()), (size_t)k);
    RawBuf text;
    size_t n = 0;
    RecordReader::slurp(path, text, n);
    std::vector<uint8_t> packed(n + 1);
    const RecordReader::Packed pk = RecordReader::parse_packed(text.data(), n, packed.data(), n + 1, least_qual);
    const Digest want = windows(packed.data(), (size_t)pk.bytes, (size_t)k);
    printf("%s : ok completed=%d pieces=%zu grows=%d puts=%d used=%" PRIu64 " cap=%zu unaligned=%d beyond=%d shrunk=%d unwritten=%" PRIu64
           " got=%" PRIu64 ",%016" PRIx64 ",%016" PRIx64 " want=%" PRIu64 ",%016" PRIx64 ",%016" PRIx64 "\n",
           line.c_str(), sink.completed, st.pieces, sink.grows, sink.puts, sink.used, sink.buf.size(), sink.unaligned, sink.beyond, sink.shrunk,
           poison, got.n, got.sum, got.x, want.n, want.sum, want.x);
}

static void plan_case(const std::string &line, std::istringstream &in)
{
    std::vector<uint64_t> bound;
    uint64_t total = 0, v;
    while (in >> v) { bound.push_back(v); total += v; }
    const uint64_t stage = stage_size(total);
    printf("%s : stage=%" PRIu64, line.c_str(), stage);
    for (const Batch &bt : plan_batches(bound, stage)) {
        printf(" | %zu %zu %" PRIu64 " %d", bt.first, bt.last, bt.bytes, (int)bt.pageable);
        for (const Slot &sl : bt.slots) printf(" %" PRIu64 ":%" PRIu64, sl.off, sl.cap);
    }
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: sketch_input_check cases.txt\n"); return 2; }
    std::ifstream cases(argv[1]);
    std::string line;
    while (std::getline(cases, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "mapped" || what == "seq") streamed_case(line, what == "mapped", in);
        else if (what == "plan") plan_case(line, in);
        else if (what == "bound") {
            std::string path;
            in >> path;
            uint64_t b = 0;
            if (packed_bound(path, b)) printf("%s : %" PRIu64 " %" PRIu64 "\n", line.c_str(), b, slot_bound(b));
            else printf("%s : unreadable\n", line.c_str());
        } else { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
