// Developer check: the section table of rk_index_blob.h as a stand-alone program (plain C++, no HIP, no GPU) -- prints, over a grid
// of dimensions, widths and flags, every offset word and the size blob_layout computes, and per present section the bytes that are
// copied and the bytes that are allocated on unpack; tests/test_blob_layout_cpu.py compares them with the rule written out in Python.
//   g++ -O1 -g -std=c++17 -Wall -Werror [-fsanitize=address,undefined] -Irabbitkssd_amd/csrc tools/blob_layout_check.cpp -o blob_layout_check && ./blob_layout_check
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "rk_index_blob.h"
int main()
{
    const uint64_t dims[] = {0, 1, 63, 64, 65, 1000};
    const uint32_t refs[] = {0, 1, 33};
    printf("header %zu magic %.8s sections %d\n", sizeof(BlobHeader), (const char *)&kBlobMagic, (int)kBlobSectionCount);
    for (uint64_t H : dims)
        for (uint64_t U : dims)
            for (uint64_t n_self : dims)
                for (uint32_t n_ref : refs)
                    for (int wide : {0, 1})
                        for (int flags = 0; flags < 8; flags++) {
                            BlobHeader h;
                            memset(&h, 0, sizeof h);
                            h.H = H;
                            h.U = U;
                            h.n_self = n_self;
                            h.n_ref = n_ref;
                            h.wide = wide;
                            h.relabeled = flags & 1;
                            h.has_src = (flags >> 1) & 1;
                            h.has_self = (flags >> 2) & 1;
                            for (const BlobSection &s : kBlobSections) h.*s.off = ~0ULL;   // (blob_layout writes every offset word)
                            blob_layout(&h);
                            printf("blob %llu %llu %llu %u %d %d :", (unsigned long long)H, (unsigned long long)U, (unsigned long long)n_self, n_ref, wide, flags);
                            for (uint64_t off : {h.off_postings, h.off_uhash, h.off_upos, h.off_sizes, h.off_self, h.off_selfoff, h.off_src, h.off_split, h.off_orig})
                                printf(" %llu", (unsigned long long)off);
                            printf(" %llu :", (unsigned long long)h.bytes);
                            for (const BlobSection &s : kBlobSections)
                                if (blob_has(h, s))
                                    printf(" %d=%llu/%llu", (int)s.id, (unsigned long long)blob_copy_bytes(h, s),
                                           (unsigned long long)((blob_dim(h, s.dim) + s.alloc) * blob_elem(h, s)));
                            printf("\n");
                        }
    return 0;
}
