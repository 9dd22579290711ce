"""CPU references for the ref-vs-query tests (tests/test_gpu_query_edges.py, tests/test_query_ref_cpu.py).

`numpy_model` restates index_dist (src/dist.cpp:560-682, :174-255 in triangle mode) with sorted postings, searchsorted
and bincount; `ref_wide` is the reference for hash spaces the dense oracle cannot hold (32-bit hashes would need a
16 GiB count array): the hashes go, widened to 64 bits, through the oracle's sparse path, and the numpy model must
agree with it field for field."""
import numpy as np

from oracle import oracle as ok


def csr(parts, dtype=np.uint32):
    """(hashes, off) of a list of per-genome arrays, as given (no sorting, repeats kept)"""
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    h = np.concatenate([np.asarray(p, dtype=dtype) for p in parts]) if parts else np.zeros(0, dtype=dtype)
    return np.ascontiguousarray(h.astype(dtype)), off


def rows_to_csr(mat, dtype=np.uint32):
    """(hashes, off) of a matrix with one genome per row: every row sorted, its repeats dropped"""
    mat = np.sort(np.asarray(mat, dtype=np.uint64), axis=1)
    keep = np.ones(mat.shape, dtype=bool)
    keep[:, 1:] = mat[:, 1:] != mat[:, :-1]
    off = np.zeros(mat.shape[0] + 1, dtype=np.uint64)
    off[1:] = np.cumsum(keep.sum(axis=1))
    return np.ascontiguousarray(mat[keep].astype(dtype)), off


def dense_reportable(triangle, max_dist):
    """is distance 1.0 (no shared hash) reported?  src/dist.cpp:232 `<` in triangle mode, :624 `<=` otherwise"""
    return 1.0 < max_dist if triangle else 1.0 <= max_dist


def numpy_model(r_hashes, r_off, q_hashes, q_off, triangle, metric, kmer_size, max_dist, rows=None, want_dense=False):
    """(hits ordered by (row, col), dense int32 [Q, R] or None; only the rows in `rows` are computed and filled).
    Every occurrence of a query hash counts every occurrence of a reference in that hash's posting list
    (src/dist.cpp:199-202 `intersectionArr[tid][curIndex]++` inside both loops)."""
    r_off = np.asarray(r_off, dtype=np.int64)
    q_off = np.asarray(q_off, dtype=np.int64)
    n_ref, n_query = len(r_off) - 1, len(q_off) - 1
    sizes = np.diff(r_off)
    gid = np.repeat(np.arange(n_ref, dtype=np.int64), sizes)
    rh = np.asarray(r_hashes).astype(np.uint64)
    order = np.lexsort((gid, rh))
    ph, pg = rh[order], gid[order]
    dense = np.zeros((n_query, n_ref), dtype=np.int32) if want_dense else None
    every = dense_reportable(triangle, max_dist)
    out = []
    for row in (range(n_query) if rows is None else rows):
        row = int(row)
        q = np.asarray(q_hashes[q_off[row]:q_off[row + 1]]).astype(np.uint64)
        lo, hi = np.searchsorted(ph, q, side="left"), np.searchsorted(ph, q, side="right")
        n = hi - lo
        at = np.repeat(lo - (np.cumsum(n) - n), n) + np.arange(int(n.sum()), dtype=np.int64)
        common = np.bincount(pg[at], minlength=n_ref).astype(np.int64)
        if want_dense:
            dense[row] = common
        first = row + 1 if triangle else 0                       # :207 / :600
        cols = np.arange(first, n_ref) if every else first + np.flatnonzero(common[first:])
        if not len(cols):
            continue
        qsize = len(q)
        c, rs = common[cols], sizes[cols]
        size0 = np.full(len(cols), qsize, dtype=np.int64) if triangle else rs      # :215-216 / :607-608
        size1 = rs if triangle else np.full(len(cols), qsize, dtype=np.int64)
        trip, inv = np.unique(np.stack([c, size0, size1], axis=1), axis=0, return_inverse=True)
        jd = np.array([ok.distance(int(t[0]), int(t[1]), int(t[2]), metric, kmer_size) for t in trip], dtype=np.float64).reshape(-1, 2)
        jorc, dist = jd[inv.reshape(-1), 0], jd[inv.reshape(-1), 1]
        keep = dist < max_dist if triangle else dist <= max_dist                   # :232 / :624
        rec = np.zeros(int(keep.sum()), dtype=ok.HIT_DTYPE)
        rec["row"], rec["col"], rec["common"] = row, cols[keep], c[keep]
        rec["size0"], rec["size1"], rec["jorc"], rec["dist"] = size0[keep], size1[keep], jorc[keep], dist[keep]
        out.append(rec)
    hits = np.concatenate(out) if out else np.zeros(0, dtype=ok.HIT_DTYPE)
    return hits, dense


def assert_same_hits(a, b, what=""):
    assert len(a) == len(b), "%s: %d hits against %d" % (what, len(a), len(b))
    for f in ("row", "col", "common", "size0", "size1", "jorc", "dist"):
        assert np.array_equal(a[f], b[f]), "%s: field %s differs" % (what, f)


def ref_wide(r_hashes, r_off, q_hashes, q_off, triangle, metric, kmer_size, max_dist, want_dense=False, threads=4):
    """reference of a hash space too large for ok.index_dist32's dense count array: the oracle's sparse (use64) path on the
    widened hashes, held equal to the numpy model"""
    r64, q64 = np.asarray(r_hashes).astype(np.uint64), np.asarray(q_hashes).astype(np.uint64)
    uhash, ucount, postings = ok.index_build64(r64, r_off)
    sizes = np.diff(np.asarray(r_off, dtype=np.int64)).astype(np.uint32)
    hits, dense = ok.index_dist64(uhash, ucount, postings, sizes, q64, q_off, triangle, metric, kmer_size, max_dist,
                                  threads=threads, want_dense=want_dense)
    m_hits, m_dense = numpy_model(r_hashes, r_off, q_hashes, q_off, triangle, metric, kmer_size, max_dist, want_dense=want_dense)
    assert_same_hits(m_hits, hits, "numpy model against ok.index_dist64")
    if want_dense:
        assert np.array_equal(m_dense, dense)
    return hits, dense
