// rk_index_io.hip -- what moves a FINISHED index in or out (the build is rk_index.hip): a translation unit of its own, so that
// a process that only imports an index from a file and joins on it does not load the code object of the build.
//   import   rk_index_import (the dense 2^bits count array of a 32-bit .index), rk_index_import64 (the sparse .index of 64-bit hashes)
//   export   rk_index_export, rk_index_export_lists, rk_index_export64: .dict / .index content in the CALLER's genome ids
//   blob     rk_index_blob_bytes, rk_index_pack_dev, rk_index_unpack_dev: one device buffer (rk_index_blob.h: header + section table)
//   copies   rk_index_broadcast: the blob over xGMI to the contexts of other devices of this process
#include <cstring>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "rk_internal.h"
#include "rk_index_blob.h"

namespace {

// a posting list that names a genome twice (or out of order): the imported index does not come from set sketches
__global__ void k_check_lists(const uint32_t *postings, const uint32_t *upos, uint64_t U, uint32_t *bad)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= U) return;
    for (uint32_t k = upos[i] + 1; k < upos[i + 1]; k++)
        if (postings[k] <= postings[k - 1]) { *bad = 1; return; }
}

// ---- import/export of the dense .index array --------------------------------------
__global__ void k_nonzero_flags(const uint32_t *counts, uint64_t n, uint32_t *flags)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = counts[i] ? 1u : 0u;
}

// rank = exclusive scan of flags, cpos = exclusive scan of counts
__global__ void k_compact_dense(const uint32_t *counts, const uint32_t *rank, const uint32_t *cpos, uint64_t n, uint32_t *uhash, uint32_t *upos)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && counts[i]) {
        uhash[rank[i]] = (uint32_t)i;
        upos[rank[i]] = cpos[i];
    }
}

__global__ void k_scatter_counts(const uint32_t *uhash, const uint32_t *upos, uint64_t U, uint32_t *counts)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < U) counts[uhash[i]] = upos[i + 1] - upos[i];
}

// ---- the sparse .index of 64-bit hashes = {u64 n; u64 hash[n]; u32 count[n]} (src/sketch.cpp:961-963, read back at
// src/dist.cpp:36-82; any block order is legal), and the same lists of a 32-bit index without its dense array
__global__ void k_counts_from_upos(const uint32_t *upos, uint64_t U, uint32_t *counts)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < U) counts[i] = upos[i + 1] - upos[i];
}

// .dict order of a renumbered index: within every list the genomes ascend by the CALLER's ids (src/sketch.cpp:979-985
// pushes genome i onto hashMapId[hash] for i ascending).  key = (list number, original id), one radix sort.
__global__ void k_export_keys(const uint32_t *postings, const uint32_t *upos, uint64_t U, uint64_t H, const uint32_t *orig,
                              unsigned long long *keys)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= H) return;
    uint64_t lo = 0, hi = U;  // largest u with upos[u] <= k
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (upos[mid] <= k) lo = mid; else hi = mid;
    }
    keys[k] = ((unsigned long long)lo << 32) | orig[postings[k]];
}
__global__ void k_low_halves(const unsigned long long *keys, uint64_t n, uint32_t *out)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = (uint32_t)keys[k];
}

// a received blob is only trusted after its payload was checked against its own header: posting ids, posting offsets, the
// genome order and every slice record must point inside the index (a corrupt record would index LDS out of range)
__global__ void k_validate_blob(const uint32_t *postings, uint64_t H, const uint32_t *upos, uint64_t U, const uint32_t *orig,
                                const uint2 *selfrange, uint64_t n_self, const uint64_t *self_off, const uint64_t *self_split,
                                uint32_t n_ref, const uint64_t *src_off, uint32_t *bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = true;
    if (i < H) ok = ok && postings[i] < n_ref;
    if (src_off && i < n_ref) ok = ok && src_off[i] <= src_off[i + 1] && src_off[i + 1] <= H && (i != 0 || src_off[0] == 0);
    if (i < U) ok = ok && upos[i] < upos[i + 1] && upos[i + 1] <= H;
    if (orig && i < n_ref) ok = ok && orig[i] < n_ref;
    if (selfrange) {
        if (i < n_self) {
            const uint2 r = selfrange[i];
            if (r.x >> 31) ok = ok && r.y != 0 && (uint64_t)(r.x & 0x7FFFFFFFu) + (31 - __clz((int)r.y)) < n_ref;
            else ok = ok && r.x < (r.y & 0x7FFFFFFFu) && (r.y & 0x7FFFFFFFu) <= H;
        }
        if (i < n_ref) ok = ok && self_off[i] <= self_split[i] && self_split[i] <= self_off[i + 1] && self_off[i + 1] <= n_self;
    }
    if (!ok) *bad = 1;
}

// ---- imports: one frame --------------------------------------------------------------------------------------------
// the index of an import with what both layouts share: dimensions, the smallest non-empty and the largest reference sketch, and
// on the context's stream the sizes and the postings (`postings`: .dict order, ascending hashes)
int begin_import(rk_ctx *ctx, const uint32_t *ref_sizes, uint32_t n_ref, const uint32_t *postings, uint64_t total, int hash_bits, bool wide,
                 IndexGuard &guard)
{
    rk_index *idx = guard.p = new (std::nothrow) rk_index;
    if (!idx) return RK_ERR_NOMEM;
    idx->ctx = ctx;
    idx->wide = wide;
    idx->n_ref = n_ref;
    idx->H = total;
    idx->hash_bits = hash_bits;
    for (uint32_t g = 0; g < n_ref; g++) {
        idx->max_ref_size = std::max<uint64_t>(idx->max_ref_size, ref_sizes[g]);
        if (ref_sizes[g] && (!idx->min_ref_size || ref_sizes[g] < idx->min_ref_size)) idx->min_ref_size = ref_sizes[g];
    }
    RK_TRY(pool_array(ctx, &idx->d_sizes, (size_t)n_ref + 1));
    RK_TRY(pool_array(ctx, &idx->d_postings, total + 8));
    RK_HIP(ctx, hipMemcpyAsync(idx->d_sizes, ref_sizes, (size_t)n_ref * 4, hipMemcpyHostToDevice, ctx->stream));
    RK_HIP(ctx, hipMemcpyAsync(idx->d_postings, postings, total * 4, hipMemcpyHostToDevice, ctx->stream));
    return RK_OK;
}

// imported index: are the posting lists strictly ascending (no genome twice)?
int classify_lists(rk_ctx *ctx, rk_index *idx, hipStream_t st)
{
    DevBuf<uint32_t> bad(ctx);
    RK_HIP(ctx, bad.alloc(1));
    RK_HIP(ctx, hipMemsetAsync(bad.p, 0, 4, st));
    if (idx->U)
        hipLaunchKernelGGL(k_check_lists, dim3(blocks_for(idx->U)), dim3(kThreads), 0, st, idx->d_postings, idx->d_upos, idx->U, bad.p);
    RK_HIP(ctx, hipGetLastError());
    uint32_t b = 0;
    RK_TRY(rk_read_back(ctx, &b, bad.p, 4, st));
    idx->ref_sets = b == 0;
    return RK_OK;
}

// ... and its end, once the lists are enqueued on `st`: synchronises (the host arrays behind the uploads may go)
int finish_import(rk_ctx *ctx, IndexGuard &guard, hipStream_t st, rk_index **out)
{
    set_dir_shape(guard.p);
    RK_TRY(classify_lists(ctx, guard.p, st));
    *out = guard.p;
    guard.p = nullptr;
    return RK_OK;
}

// ---- exports: one tail ---------------------------------------------------------------------------------------------
// the postings as the .dict file lists them, in a pool buffer the caller frees (null: the index's own array already is)
int postings_in_caller_ids(rk_ctx *ctx, const rk_index *idx, hipStream_t st, uint32_t **out)
{
    *out = nullptr;
    if (!idx->relabeled || !idx->H) return RK_OK;
    DevBuf<unsigned long long> keys(ctx), sorted(ctx);
    DevBuf<uint32_t> res(ctx);
    RK_HIP(ctx, keys.alloc(idx->H));
    RK_HIP(ctx, sorted.alloc(idx->H));
    RK_HIP(ctx, res.alloc(idx->H));
    int ubits = 1;
    while (ubits < 32 && (1ULL << ubits) < idx->U) ubits++;
    hipLaunchKernelGGL(k_export_keys, dim3(blocks_for(idx->H)), dim3(kThreads), 0, st, idx->d_postings, idx->d_upos, idx->U, idx->H,
                       idx->d_orig, keys.p);
    RK_TRY(rk_prim_sort_keys_u64(ctx, keys.p, sorted.p, idx->H, 0, (unsigned)(32 + ubits), st));
    hipLaunchKernelGGL(k_low_halves, dim3(blocks_for(idx->H)), dim3(kThreads), 0, st, sorted.p, idx->H, res.p);
    RK_HIP(ctx, hipGetLastError());
    RK_HIP(ctx, hipStreamSynchronize(st));  // the temporaries return to the pool
    *out = res.release();
    return RK_OK;
}

// ... on the host (every export): synchronises when there is something to copy
int download_postings(rk_ctx *ctx, const rk_index *idx, hipStream_t st, uint32_t *postings)
{
    if (!postings || !idx->H) return RK_OK;
    DevBuf<uint32_t> mapped(ctx);
    RK_TRY(postings_in_caller_ids(ctx, idx, st, &mapped.p));
    RK_HIP(ctx, hipMemcpyAsync(postings, mapped.p ? mapped.p : idx->d_postings, idx->H * 4, hipMemcpyDeviceToHost, st));
    RK_HIP(ctx, hipStreamSynchronize(st));
    return RK_OK;
}

// rk_index_export_lists and rk_index_export64 behind their refusals: the lists without a dense array, over the width of the hashes
template <class Hash> int export_lists(const rk_index *idx, const Hash *d_uhash, uint32_t *postings, Hash *hashes, uint32_t *counts)
{
    rk_ctx *ctx = idx->ctx;
    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RK_TRY(download_postings(ctx, idx, st, postings));
    if (hashes && idx->U) RK_HIP(ctx, hipMemcpyAsync(hashes, d_uhash, idx->U * sizeof(Hash), hipMemcpyDeviceToHost, st));
    DevBuf<uint32_t> c(ctx);
    if (counts && idx->U) {
        RK_HIP(ctx, c.alloc(idx->U));
        hipLaunchKernelGGL(k_counts_from_upos, dim3(blocks_for(idx->U)), dim3(kThreads), 0, st, idx->d_upos, idx->U, c.p);
        RK_HIP(ctx, hipGetLastError());
        RK_HIP(ctx, hipMemcpyAsync(counts, c.p, idx->U * 4, hipMemcpyDeviceToHost, st));
    }
    RK_HIP(ctx, hipStreamSynchronize(st));
    return RK_OK;
}

// ---- the blob: rk_index_blob.h says what travels, this binds a section to its array in the index (f sees the member itself) ----
template <class Index, class F> int with_section(Index *idx, BlobSectionId id, F f)
{
    switch (id) {
    case kSecPostings: return f(idx->d_postings);
    case kSecUhash: return idx->wide ? f(idx->d_uhash64) : f(idx->d_uhash);
    case kSecUpos: return f(idx->d_upos);
    case kSecSizes: return f(idx->d_sizes);
    case kSecOrig: return f(idx->d_orig);
    case kSecSrc: return f(idx->d_src_off);
    case kSecSelf: return f(idx->d_selfrange);
    case kSecSelfOff: return f(idx->d_self_off);
    case kSecSplit: return f(idx->d_self_split);
    default: return RK_ERR_ARG;
    }
}

void blob_header(const rk_index *idx, BlobHeader *h)
{
    memset(h, 0, sizeof(*h));
    h->magic = kBlobMagic;
    h->H = idx->H;
    h->U = idx->U;
    h->max_src_size = idx->max_src_size;
    h->max_ref_size = idx->max_ref_size;
    h->min_ref_size = idx->min_ref_size;
    h->n_self = idx->n_self;
    h->n_ref = idx->n_ref;
    h->has_self = idx->d_selfrange ? 1 : 0;
    h->has_src = idx->d_src_off ? 1 : 0;
    h->ref_sets = idx->ref_sets ? 1 : 0;
    h->relabeled = idx->relabeled && idx->d_orig ? 1 : 0;
    h->hash_bits = idx->hash_bits;
    h->wide = idx->wide ? 1 : 0;
    blob_layout(h);
}

}  // namespace

extern "C" {

int rk_index_import(rk_ctx *ctx, const uint32_t *postings, uint64_t total, const uint32_t *counts, int hash_bits, const uint32_t *ref_sizes, uint32_t n_ref, rk_index **out)
{
    if (!ctx || !out || !counts || (!postings && total) || (!ref_sizes && n_ref)) return RK_ERR_ARG;
    *out = nullptr;
    if (hash_bits < 1 || hash_bits > 32) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "hash_bits=%d outside the 32-bit layout", hash_bits);
    if (total >= 0xFFFFFFFFULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "more than 2^32-1 postings");
    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t hs = 1ULL << hash_bits;
    IndexGuard guard{nullptr};
    RK_TRY(begin_import(ctx, ref_sizes, n_ref, postings, total, hash_bits, false, guard));
    rk_index *idx = guard.p;
    DevBuf<uint32_t> d_counts(ctx), flags(ctx), rank(ctx), cpos(ctx), last_dev(ctx);
    for (DevBuf<uint32_t> *buf : {&d_counts, &flags, &rank, &cpos}) RK_HIP(ctx, buf->alloc(hs));
    RK_HIP(ctx, hipMemcpyAsync(d_counts.p, counts, hs * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_nonzero_flags, dim3(blocks_for(hs)), dim3(kThreads), 0, st, d_counts.p, hs, flags.p);
    RK_TRY(rk_prim_exclusive_scan_u32(ctx, flags.p, rank.p, hs, st));
    RK_TRY(rk_prim_exclusive_scan_u32(ctx, d_counts.p, cpos.p, hs, st));
    uint32_t last[4] = {0, 0, 0, 0};  // rank, flag, cpos, count of the last hash value
    const uint32_t *const ends[4] = {rank.p, flags.p, cpos.p, d_counts.p};
    RK_HIP(ctx, last_dev.alloc(4));
    for (int i = 0; i < 4; i++) RK_HIP(ctx, hipMemcpyAsync(last_dev.p + i, ends[i] + (hs - 1), 4, hipMemcpyDeviceToDevice, st));
    RK_TRY(rk_read_back(ctx, last, last_dev.p, 16, st));
    idx->U = (uint64_t)last[0] + last[1];
    if ((uint64_t)last[2] + last[3] != total)  // src/dist.cpp:107-110
        return rk_fail(ctx, RK_ERR_ARG, "mismatched total hash number: index says %llu, dict has %llu",
                       (unsigned long long)last[2] + last[3], (unsigned long long)total);
    RK_TRY(pool_array(ctx, &idx->d_uhash, idx->U + 1));
    RK_TRY(pool_array(ctx, &idx->d_upos, idx->U + 2));
    hipLaunchKernelGGL(k_compact_dense, dim3(blocks_for(hs)), dim3(kThreads), 0, st, d_counts.p, rank.p, cpos.p, hs, idx->d_uhash, idx->d_upos);
    const uint32_t tot32 = (uint32_t)total;
    memcpy(ctx->pinned, &tot32, 4);
    RK_HIP(ctx, hipMemcpyAsync(idx->d_upos + idx->U, ctx->pinned, 4, hipMemcpyHostToDevice, st));
    RK_HIP(ctx, hipGetLastError());
    return finish_import(ctx, guard, st, out);
}

int rk_index_import64(rk_ctx *ctx, const uint32_t *postings, uint64_t total, const uint64_t *hashes,
                      const uint32_t *counts, uint64_t n_hash, int hash_bits, const uint32_t *ref_sizes,
                      uint32_t n_ref, rk_index **out)
{
    if (!ctx || !out || (!postings && total) || ((!hashes || !counts) && n_hash) || (!ref_sizes && n_ref)) return RK_ERR_ARG;
    *out = nullptr;
    if (hash_bits <= 32 || hash_bits > 64) return rk_fail(ctx, RK_ERR_ARG, "hash_bits=%d is not a 64-bit layout", hash_bits);
    if (total >= 0xFFFFFFFFULL || n_hash >= 0xFFFFFFFFULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "more than 2^32-1 postings");
    // the file may list the posting blocks in any order (the reference writes hash-map order):
    // bring them into ascending hash order on the host, then upload
    std::vector<uint64_t> start(n_hash + 1, 0);
    for (uint64_t i = 0; i < n_hash; i++) start[i + 1] = start[i] + counts[i];
    if (start[n_hash] != total)
        return rk_fail(ctx, RK_ERR_ARG, "mismatched total hash number: index says %llu, dict has %llu",
                       (unsigned long long)start[n_hash], (unsigned long long)total);
    std::vector<uint32_t> order(n_hash);
    for (uint64_t i = 0; i < n_hash; i++) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hashes[a] < hashes[b]; });
    std::vector<uint64_t> uh(n_hash + 1);
    std::vector<uint32_t> up(n_hash + 2, 0), post(total + 1);
    uint64_t w = 0;
    for (uint64_t r = 0; r < n_hash; r++) {
        const uint32_t i = order[r];
        if (r && hashes[i] == uh[r - 1]) return rk_fail(ctx, RK_ERR_ARG, "duplicate hash in the index file");
        uh[r] = hashes[i];
        up[r] = (uint32_t)w;
        memcpy(post.data() + w, postings + start[i], (size_t)counts[i] * 4);
        w += counts[i];
    }
    up[n_hash] = (uint32_t)w;
    RK_HIP(ctx, hipSetDevice(ctx->device));
    IndexGuard guard{nullptr};
    RK_TRY(begin_import(ctx, ref_sizes, n_ref, post.data(), total, hash_bits, true, guard));
    rk_index *idx = guard.p;
    idx->U = n_hash;
    hipStream_t st = ctx->stream;
    RK_TRY(pool_array(ctx, &idx->d_uhash64, n_hash + 1));
    RK_TRY(pool_array(ctx, &idx->d_upos, n_hash + 2));
    RK_HIP(ctx, hipMemcpyAsync(idx->d_uhash64, uh.data(), n_hash * 8, hipMemcpyHostToDevice, st));
    RK_HIP(ctx, hipMemcpyAsync(idx->d_upos, up.data(), (n_hash + 1) * 4, hipMemcpyHostToDevice, st));
    return finish_import(ctx, guard, st, out);
}

int rk_index_export(const rk_index *idx, uint32_t *postings, uint32_t *counts)
{
    if (!idx) return RK_ERR_ARG;
    rk_ctx *ctx = idx->ctx;
    if (idx->wide && counts) return rk_fail(ctx, RK_ERR_ARG, "64-bit index: use rk_index_export64 (sparse .index layout)");
    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RK_TRY(download_postings(ctx, idx, st, postings));
    if (counts) {
        const uint64_t hs = 1ULL << idx->hash_bits;
        DevBuf<uint32_t> d_counts(ctx);
        RK_HIP(ctx, d_counts.alloc(hs));
        RK_HIP(ctx, hipMemsetAsync(d_counts.p, 0, hs * 4, st));
        if (idx->U)
            hipLaunchKernelGGL(k_scatter_counts, dim3(blocks_for(idx->U)), dim3(kThreads), 0, st, idx->d_uhash, idx->d_upos, idx->U, d_counts.p);
        RK_HIP(ctx, hipGetLastError());
        RK_HIP(ctx, hipMemcpyAsync(counts, d_counts.p, hs * 4, hipMemcpyDeviceToHost, st));
        RK_HIP(ctx, hipStreamSynchronize(st));
    }
    RK_HIP(ctx, hipStreamSynchronize(st));
    return RK_OK;
}

int rk_index_export_lists(const rk_index *idx, uint32_t *postings, uint32_t *hashes, uint32_t *counts)
{
    if (!idx) return RK_ERR_ARG;
    if (idx->wide) return rk_fail(idx->ctx, RK_ERR_ARG, "64-bit index: use rk_index_export64");
    return export_lists(idx, idx->d_uhash, postings, hashes, counts);
}

int rk_index_export64(const rk_index *idx, uint32_t *postings, uint64_t *hashes, uint32_t *counts)
{
    if (!idx) return RK_ERR_ARG;
    if (!idx->wide) return rk_fail(idx->ctx, RK_ERR_ARG, "32-bit index: use rk_index_export (dense .index layout)");
    return export_lists(idx, idx->d_uhash64, postings, hashes, counts);
}

uint64_t rk_index_blob_bytes(const rk_index *idx)
{
    if (!idx) return 0;
    BlobHeader h;
    blob_header(idx, &h);
    return h.bytes;
}

int rk_index_pack_dev(const rk_index *idx, void *blob_dev, uint64_t blob_cap, void *stream_v)
{
    if (!idx || !blob_dev) return RK_ERR_ARG;
    rk_ctx *ctx = idx->ctx;
    hipStream_t st = (hipStream_t)stream_v;
    BlobHeader h;
    blob_header(idx, &h);
    if (blob_cap < h.bytes) return rk_fail(ctx, RK_ERR_CAPACITY, "blob needs %llu bytes", (unsigned long long)h.bytes);
    char *b = (char *)blob_dev;
    RK_HIP(ctx, hipSetDevice(ctx->device));
    RK_HIP(ctx, hipMemcpyAsync(b, &h, sizeof(h), hipMemcpyHostToDevice, st));
    for (const BlobSection &s : kBlobSections)
        if (blob_has(h, s))
            RK_TRY(with_section(idx, s.id, [&](const auto *arr) -> int {
                RK_HIP(ctx, hipMemcpyAsync(b + h.*s.off, arr, blob_copy_bytes(h, s), hipMemcpyDeviceToDevice, st));
                return RK_OK;
            }));
    RK_HIP(ctx, hipStreamSynchronize(st));
    return RK_OK;
}

int rk_index_unpack_dev(rk_ctx *ctx, const void *blob_dev, uint64_t blob_bytes, void *stream_v, rk_index **out)
{
    if (!ctx || !blob_dev || !out || blob_bytes < sizeof(BlobHeader)) return RK_ERR_ARG;
    *out = nullptr;
    hipStream_t st = (hipStream_t)stream_v;
    RK_HIP(ctx, hipSetDevice(ctx->device));
    BlobHeader h;
    RK_HIP(ctx, hipMemcpyAsync(&h, blob_dev, sizeof(h), hipMemcpyDeviceToHost, st));
    RK_HIP(ctx, hipStreamSynchronize(st));
    // the offsets must be exactly the ones this library computes for the stated dimensions, and fit the buffer:
    // a truncated or foreign blob is rejected before any copy is sized from it
    BlobHeader chk = h;
    blob_layout(&chk);
    if (h.magic != kBlobMagic || h.H >= 0xFFFFFFFFULL || h.U > h.H || h.hash_bits < 1 || h.hash_bits > 64 ||
        (h.wide != 0) != (h.hash_bits > 32) || memcmp(&chk, &h, sizeof(h)) != 0 || h.bytes > blob_bytes)
        return rk_fail(ctx, RK_ERR_ARG, "not an index blob of this library (or truncated: %llu of %llu bytes)",
                       (unsigned long long)blob_bytes, (unsigned long long)h.bytes);
    rk_index *idx = new (std::nothrow) rk_index;
    if (!idx) return RK_ERR_NOMEM;
    IndexGuard guard{idx};
    idx->ctx = ctx;
    idx->n_ref = h.n_ref;
    idx->H = h.H;
    idx->U = h.U;
    idx->max_src_size = h.max_src_size;
    idx->max_ref_size = h.max_ref_size;
    idx->min_ref_size = h.min_ref_size;
    idx->n_self = h.n_self;
    idx->ref_sets = h.ref_sets != 0;
    idx->relabeled = h.relabeled != 0;
    idx->hash_bits = h.hash_bits;
    idx->wide = h.wide != 0;
    set_dir_shape(idx);
    const char *b = (const char *)blob_dev;
    // (an index without slice records -- built with tile records -- still self joins when the offsets of its source sketches
    // came along: its tile records are rebuilt on first use)
    for (const BlobSection &s : kBlobSections)
        if (blob_has(h, s))
            RK_TRY(with_section(idx, s.id, [&](auto *&arr) -> int {
                RK_TRY(pool_array(ctx, &arr, blob_dim(h, s.dim) + s.alloc));
                RK_HIP(ctx, hipMemcpyAsync(arr, b + h.*s.off, blob_copy_bytes(h, s), hipMemcpyDeviceToDevice, st));
                return RK_OK;
            }));
    {
        DevBuf<uint32_t> bad(ctx);
        RK_HIP(ctx, bad.alloc(1));
        RK_HIP(ctx, hipMemsetAsync(bad.p, 0, 4, st));
        const uint64_t span = std::max<uint64_t>(std::max<uint64_t>(idx->H, idx->n_self), (uint64_t)idx->n_ref + 1);
        if (span)
            hipLaunchKernelGGL(k_validate_blob, dim3(blocks_for(span)), dim3(kThreads), 0, st, idx->d_postings, idx->H, idx->d_upos, idx->U,
                               idx->relabeled ? idx->d_orig : nullptr, idx->d_selfrange, idx->n_self, idx->d_self_off, idx->d_self_split,
                               idx->n_ref, idx->d_src_off, bad.p);
        RK_HIP(ctx, hipGetLastError());
        uint32_t b = 0;
        RK_TRY(rk_read_back(ctx, &b, bad.p, 4, st));  // synchronises: the copies above are complete
        if (b) return rk_fail(ctx, RK_ERR_ARG, "index blob payload is inconsistent with its header (corrupt or foreign blob)");
    }
    guard.p = nullptr;
    *out = idx;
    return RK_OK;
}

}  // extern "C"

// ---- one-to-all replication inside one process (the host tool's --gpus N) -----------------------------------
static constexpr int kPeerCopyTimeoutS = 120;
extern "C" int rk_index_broadcast(const rk_index *src, rk_ctx *const *dst, uint32_t n_dst, rk_index **out)
{
    if (!src || (n_dst && (!dst || !out))) return RK_ERR_ARG;
    rk_ctx *sctx = src->ctx;
    for (uint32_t i = 0; i < n_dst; i++) out[i] = nullptr;
    if (!n_dst) return RK_OK;
    const uint64_t bytes = rk_index_blob_bytes(src);
    RK_HIP(sctx, hipSetDevice(sctx->device));
    DevBuf<char> blob(sctx);
    if (blob.alloc(bytes) != hipSuccess) return rk_fail(sctx, RK_ERR_NOMEM, "cannot allocate the %llu-byte index blob", (unsigned long long)bytes);
    int rc = rk_index_pack_dev(src, blob.p, bytes, sctx->stream);  // synchronises the source stream
    if (rc) return rc;
    // every peer pulls the blob over its own xGMI link at the same time (the links are point to point, so a
    // one-to-all of direct copies moves the blob once per link, like a pipelined ring, without a communicator)
    std::vector<char *> peer(n_dst, nullptr);
    for (uint32_t i = 0; i < n_dst; i++)
        if (!dst[i]) return RK_ERR_ARG;
    // error exit: copies already enqueued into the first n peer blobs may still be running -- wait for them before the
    // blocks return to their pools (a later allocation could receive a block that is still being written), and leave
    // the caller's device current
    auto abandon = [&](uint32_t n) {
        for (uint32_t j = 0; j < n; j++) {
            if (!peer[j]) continue;
            if (hipSetDevice(dst[j]->device) == hipSuccess) (void)hipStreamSynchronize(dst[j]->stream);
            rk_pool_free(dst[j], peer[j]);
        }
        (void)hipGetLastError();
        (void)hipSetDevice(sctx->device);
    };
    for (uint32_t i = 0; i < n_dst; i++) {
        rk_ctx *d = dst[i];
        if (hipSetDevice(d->device) != hipSuccess) {
            abandon(i);
            return rk_fail(d, RK_ERR_HIP, "cannot select device %d", d->device);
        }
        peer[i] = static_cast<char *>(rk_pool_alloc(d, bytes));
        if (!peer[i]) {
            abandon(i);
            return rk_fail(d, RK_ERR_NOMEM, "cannot allocate the %llu-byte index blob on device %d", (unsigned long long)bytes, d->device);
        }
        hipError_t e;
        if (d->device == sctx->device) {
            e = hipMemcpyAsync(peer[i], blob.p, bytes, hipMemcpyDeviceToDevice, d->stream);
        } else {
            int can = 0;
            (void)hipDeviceCanAccessPeer(&can, d->device, sctx->device);
            if (can) {
                hipError_t pe = hipDeviceEnablePeerAccess(sctx->device, 0);
                if (pe != hipSuccess) (void)hipGetLastError();  // already enabled
            }
            e = hipMemcpyPeerAsync(peer[i], d->device, blob.p, sctx->device, bytes, d->stream);
        }
        if (e != hipSuccess) {
            abandon(i + 1);
            return rk_fail(d, RK_ERR_HIP, "index copy to device %d failed: %s", d->device, hipGetErrorString(e));
        }
    }
    bool stuck = false;  // a copy that never completed: its blocks are leaked rather than waited for
    for (uint32_t i = 0; i < n_dst && !rc; i++) {
        rk_ctx *d = dst[i];
        // bounded wait: a peer copy that never completes (a link that is down) must end in an error, not in a hang
        hipError_t qe = hipSetDevice(d->device);
        const auto t_start = std::chrono::steady_clock::now();
        while (qe == hipSuccess) {
            qe = hipStreamQuery(d->stream);
            if (qe != hipErrorNotReady) break;
            if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(kPeerCopyTimeoutS)) break;
            std::this_thread::sleep_for(std::chrono::microseconds(50));
            qe = hipSuccess;
        }
        (void)hipGetLastError();  // (hipStreamQuery's hipErrorNotReady is sticky for the next hipGetLastError check)
        if (qe == hipErrorNotReady) stuck = true;
        if (qe == hipErrorNotReady)
            rc = rk_fail(d, RK_ERR_HIP, "index copy of %llu bytes from device %d to device %d did not complete within %d s", (unsigned long long)bytes,
                         sctx->device, d->device, kPeerCopyTimeoutS);
        else if (qe != hipSuccess)
            rc = rk_fail(d, RK_ERR_HIP, "index copy to device %d failed: %s", d->device, hipGetErrorString(qe));
        else
            rc = rk_index_unpack_dev(d, peer[i], bytes, d->stream, &out[i]);
    }
    if (rc) {
        // the caller asks the SOURCE context for the message: carry the failing peer's text over
        for (uint32_t i = 0; i < n_dst; i++)
            if (dst[i] != sctx && !dst[i]->err.empty()) sctx->err = "device " + std::to_string(dst[i]->device) + ": " + dst[i]->err;
        if (!stuck) abandon(n_dst);  // waits for the copies of the peers behind the failing one
        else (void)hipSetDevice(sctx->device);
        for (uint32_t i = 0; i < n_dst; i++) {
            rk_index_free(out[i]);
            out[i] = nullptr;
        }
        return rc;
    }
    for (uint32_t i = 0; i < n_dst; i++) rk_pool_free(dst[i], peer[i]);
    (void)hipSetDevice(sctx->device);
    return rc;
}
