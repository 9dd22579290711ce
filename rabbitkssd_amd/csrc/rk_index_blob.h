// rk_index_blob.h -- the single-buffer form of an index (rk_index_pack_dev / rk_index_unpack_dev, rk_index_broadcast, the RCCL
// broadcast of shard.py): a header, then the sections of kBlobSections, each 256-byte aligned, in the table's order.  Plain C++
// without HIP types (tools/blob_layout_check.cpp compiles it alone).
//
// The table is the ONE place that says what travels: blob_layout, the copies of rk_index_pack_dev and the allocations and copies
// of rk_index_unpack_dev are loops over it.  A new array is a new offset word at the END of the header (and a new magic: old
// blobs must be refused), a row here, and its binding to the rk_index member in rk_index_io.hip (with_section).  Derived arrays
// -- prefix directory, rank bitmap, tile records -- are not shipped: every rank rebuilds them on first use.
#pragma once
#include <cstddef>
#include <cstdint>

struct BlobHeader {
    uint64_t magic, bytes;
    uint64_t H, U, max_src_size, max_ref_size, min_ref_size, n_self;
    uint32_t n_ref, has_self, ref_sets, relabeled;
    int32_t hash_bits, wide, has_src;   // has_src: the CSR offsets of the source sketches travel (an index built here: it can self join)
    uint64_t off_postings, off_uhash, off_upos, off_sizes, off_self, off_selfoff, off_src, off_split, off_orig;
};
static_assert(sizeof(BlobHeader) == 168, "the header is part of the wire format");
constexpr uint64_t kBlobMagic = 0x37584449444b5352ULL;  // "RSKDIDX7"
inline uint64_t al256(uint64_t x) { return (x + 255) & ~255ULL; }

enum BlobSectionId { kSecPostings, kSecUhash, kSecUpos, kSecSizes, kSecOrig, kSecSrc, kSecSelf, kSecSelfOff, kSecSplit, kBlobSectionCount };
enum BlobDim { kDimH, kDimU, kDimRef, kDimSelf };            // the header's H, U, n_ref, n_self
enum BlobWhen { kAlways, kIfRelabeled, kIfSrc, kIfSelf };    // the header's relabeled, has_src, has_self

// One section: `dim` + reserve elements of room in the blob, dim + copy of them carried, dim + alloc allocated on unpack.
// (postings: padded to H + 8 in the index, the kernels read up to eight postings from any list start; upos: its U + 1 offsets
// travel; the per-genome u32 arrays travel without their spare element, the u64 offset arrays with it)
struct BlobSection {
    BlobSectionId id;
    uint64_t BlobHeader::*off;       // its offset word in the header (0: the section is absent)
    uint32_t elem, elem_wide;        // bytes per element, and with 64-bit hashes
    BlobDim dim;
    uint32_t reserve, copy, alloc;
    BlobWhen when;
};
constexpr BlobSection kBlobSections[kBlobSectionCount] = {
    {kSecPostings, &BlobHeader::off_postings, 4, 4, kDimH, 1, 0, 8, kAlways},
    {kSecUhash, &BlobHeader::off_uhash, 4, 8, kDimU, 1, 0, 1, kAlways},
    {kSecUpos, &BlobHeader::off_upos, 4, 4, kDimU, 2, 1, 2, kAlways},
    {kSecSizes, &BlobHeader::off_sizes, 4, 4, kDimRef, 1, 0, 1, kAlways},
    {kSecOrig, &BlobHeader::off_orig, 4, 4, kDimRef, 1, 0, 1, kIfRelabeled},
    {kSecSrc, &BlobHeader::off_src, 8, 8, kDimRef, 1, 1, 1, kIfSrc},
    {kSecSelf, &BlobHeader::off_self, 8, 8, kDimSelf, 1, 0, 1, kIfSelf},
    {kSecSelfOff, &BlobHeader::off_selfoff, 8, 8, kDimRef, 1, 1, 1, kIfSelf},
    {kSecSplit, &BlobHeader::off_split, 8, 8, kDimRef, 1, 1, 1, kIfSelf},
};

inline uint64_t blob_dim(const BlobHeader &h, BlobDim d) { return d == kDimH ? h.H : d == kDimU ? h.U : d == kDimRef ? h.n_ref : h.n_self; }
inline bool blob_has(const BlobHeader &h, const BlobSection &s)
{
    return s.when == kAlways || (s.when == kIfRelabeled && h.relabeled) || (s.when == kIfSrc && h.has_src) || (s.when == kIfSelf && h.has_self);
}
inline uint64_t blob_elem(const BlobHeader &h, const BlobSection &s) { return h.wide ? s.elem_wide : s.elem; }
inline uint64_t blob_copy_bytes(const BlobHeader &h, const BlobSection &s) { return (blob_dim(h, s.dim) + s.copy) * blob_elem(h, s); }

// the layout this library produces for an index of the header's dimensions and flags: every offset word and `bytes`
inline void blob_layout(BlobHeader *h)
{
    uint64_t p = al256(sizeof(BlobHeader));
    for (const BlobSection &s : kBlobSections) {
        h->*s.off = 0;
        if (!blob_has(*h, s)) continue;
        h->*s.off = p;
        p = al256(p + (blob_dim(*h, s.dim) + s.reserve) * blob_elem(*h, s));
    }
    h->bytes = p;
}
