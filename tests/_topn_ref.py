"""`dist -N` from the hash sets, independent of the library: per cell `common` from np.intersect1d and the sizes from the sets, jorc
and dist in float64 in the operation order of rk_distance (host_distance of tests/test_topn_cpu.py), the stream = the cells with
dist <= D in column order, the heap = the oracle's (ok.topn_row).  Output: HIT_DTYPE records per selected row, in pop order.

One thing host_distance leaves open: numpy's vector log differs from the C library's in the last bit on some CPUs and inputs (about
one argument in 300 where it was tried), and the reference program -- and the library's host finish -- call the C library's.  The
records here are bit for bit, so distances() takes the log of every distinct argument again with math.log, which is the C library's.

Also here: the builder of reference sets with prescribed cells (build_refs), and the rows of a block-cyclic shard."""
import math

import numpy as np

from oracle import oracle as ok
from rabbitkssd_amd import capi
from test_topn_cpu import host_distance


def distances(common, size0, size1, metric, k):
    """(jorc, dist) of cells, float64: host_distance with the C library's log"""
    common, size0, size1 = (np.asarray(x, dtype=np.int64) for x in (common, size0, size1))
    j, d = host_distance(common, size0, size1, metric, k)
    j, d = np.array(j, dtype=np.float64), np.array(d, dtype=np.float64)
    logged = (j > 0.0) & (j < 1.0)
    x = j[logged] if metric else (2 * j[logged]) / (1.0 + j[logged])
    ux, inv = np.unique(x, return_inverse=True)
    exact = np.array([(-1.0 / k) * math.log(v) for v in ux.tolist()], dtype=np.float64)
    d[logged] = exact[inv] if len(ux) else exact
    return j, d


def cells(refs, queries):
    """(common int64[Q, R], size0 int64[R], size1 int64[Q]) of hash sets given as arrays without repeats"""
    common = np.zeros((len(queries), len(refs)), dtype=np.int64)
    for qi, q in enumerate(queries):
        if len(q):
            for ri, r in enumerate(refs):
                if len(r):
                    common[qi, ri] = len(np.intersect1d(q, r, assume_unique=True))
    return common, np.array([len(r) for r in refs], dtype=np.int64), np.array([len(q) for q in queries], dtype=np.int64)


def row_records(row, common, size0, size1, metric, k):
    """every cell of one row as HIT_DTYPE, in column order"""
    R = len(common)
    rec = np.zeros(R, dtype=capi.HIT_DTYPE)
    rec["row"], rec["col"] = row, np.arange(R)
    rec["common"], rec["size0"], rec["size1"] = common, size0, size1
    rec["jorc"], rec["dist"] = distances(common, size0, np.full(R, size1), metric, k)
    return rec


def reference(cell, metric, k, D, N, rows=None):
    """cell = cells(refs, queries); rows: the selected query rows, ascending (default all)"""
    common, size0, size1 = cell
    out = [np.zeros(0, dtype=capi.HIT_DTYPE)]
    for q in (range(len(size1)) if rows is None else rows):
        rec = row_records(q, common[q], size0, int(size1[q]), metric, k)
        out.append(ok.topn_row(rec[rec["dist"] <= D], N))   # src/dist.cpp:624: the stream, non-strict
    return np.concatenate(out)


def shard_rows(n_query, row_first=0, row_step=1, row_block=0):
    """the rows of a shard: blocks of row_block rows dealt round-robin from block row_first, as rk_dist_opts"""
    rb, rs = max(1, row_block), max(1, row_step)
    return [r for r in range(n_query) if r // rb >= row_first and (r // rb - row_first) % rs == 0]


class Pool:
    """distinct hashes of `bits` bits: take(n) never returns a hash twice (an odd multiplier permutes the residues mod 2^bits)"""
    def __init__(self, bits, seed):
        self.bits, self.next = bits, 0
        rng = np.random.default_rng(seed)
        self.mult = int(rng.integers(1 << (bits - 2), 1 << (bits - 1))) * 2 + 1
        self.add = int(rng.integers(0, 1 << bits))

    def take(self, n):
        assert self.next + n <= 1 << self.bits
        i = np.arange(self.next, self.next + n, dtype=np.uint64)
        self.next += n
        # (uint64 arrays wrap mod 2^64, of which 2^bits is a divisor: the residues are exact)
        return (i * np.uint64(self.mult) + np.uint64(self.add)) & np.uint64((1 << self.bits) - 1)


def build_refs(pool, rng, queries, common, sizes):
    """Reference sets with prescribed cells.  queries: hash arrays that share no hash with each other (all from `pool`);
    common[q][j]: how many hashes reference j shares with query q; sizes[j]: its size.  Reference j holds common[q][j] hashes of
    every query q, drawn at random per column (not a prefix), and sizes[j] - sum_q common[q][j] private hashes that no other sketch
    holds.  Returns the references as sorted arrays of the pool's dtype (uint64)."""
    common = np.asarray(common, dtype=np.int64).reshape(len(queries), len(sizes))
    refs = []
    for j, size in enumerate(sizes):
        shared = int(common[:, j].sum())
        assert 0 <= shared <= size and all(common[q, j] <= len(queries[q]) for q in range(len(queries))), (j, size, common[:, j])
        parts = [rng.choice(queries[q], size=int(common[q, j]), replace=False) for q in range(len(queries)) if common[q, j]]
        parts.append(pool.take(int(size) - shared))
        refs.append(np.sort(np.concatenate(parts)).astype(np.uint64))
    return refs
