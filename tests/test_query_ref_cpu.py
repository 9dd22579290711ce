"""The numpy model of tests/_query_ref.py -- the second reference of the 32-bit-hash query tests -- against the oracle
(ok.index_dist32, and ok.index_dist64 on the widened hashes), field for field.  No GPU."""
import numpy as np
import pytest

from oracle import oracle as ok
from rabbitkssd_amd import synth

import _query_ref as qr


def shape(n_ref, m, bits, seed):
    """references in clades, one repeating hashes and one empty; queries: a copy of a reference, parts of two references,
    a query that repeats hashes, an empty and a one-hash query, an unrelated one and relatives with foreign hashes"""
    _, rh, roff = synth.clade_sketches(n_ref, m, bits, seed=seed)
    parts = [rh[int(roff[i]):int(roff[i + 1])] for i in range(n_ref)]
    parts[3] = np.sort(np.concatenate([parts[3], parts[3][:5]]))          # a multiset reference (src/dist.cpp:199-202 counts both)
    parts[n_ref - 1] = np.zeros(0, dtype=np.uint32)                       # an empty reference
    rh, roff = qr.csr(parts)
    rng = np.random.default_rng(seed + 100)
    q = [parts[0], np.concatenate([parts[3][::2], parts[14]]), np.repeat(parts[7][:20], 3), np.zeros(0, dtype=np.uint32),
         parts[5][:1], rng.integers(0, 1 << bits, size=m, dtype=np.uint64).astype(np.uint32)]
    q += [np.unique(np.concatenate([parts[int(r)][: m // 2], rng.integers(0, 1 << bits, size=m // 3, dtype=np.uint64).astype(np.uint32)]))
          for r in rng.integers(0, n_ref, size=10)]
    qh, qoff = qr.csr(q)
    return rh, roff, qh, qoff


@pytest.mark.parametrize("n_ref,m,bits,seed", [(60, 40, 20, 1), (200, 25, 22, 2), (35, 300, 24, 3)])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("max_dist", [0.08, 1.5])
def test_numpy_model_equals_the_oracle(n_ref, m, bits, seed, metric, max_dist):
    rh, roff, qh, qoff = shape(n_ref, m, bits, seed)
    postings, counts = ok.index_build32(rh, roff, bits)
    sizes = np.diff(roff).astype(np.uint32)
    # triangle 0: explicit queries; triangle 1: the indexed sketches as queries
    for triangle, (xh, xoff) in ((0, (qh, qoff)), (1, (rh, roff))):
        want, wdense = ok.index_dist32(counts, bits, postings, sizes, xh, xoff, triangle, metric, 20, max_dist, want_dense=True)
        mine, dense = qr.numpy_model(rh, roff, xh, xoff, triangle, metric, 20, max_dist, want_dense=True)
        assert len(want) > 0
        qr.assert_same_hits(mine, want, "triangle=%d" % triangle)
        assert np.array_equal(dense, wdense)
        # a subset of the rows (what a block-cyclic shard computes)
        rows = list(range(1, len(xoff) - 1, 3))
        part, _ = qr.numpy_model(rh, roff, xh, xoff, triangle, metric, 20, max_dist, rows=rows)
        qr.assert_same_hits(part, want[np.isin(want["row"], rows)], "rows")
        # the sparse oracle on the widened hashes (the route of 32-bit hash spaces) agrees as well
        wide, wd = qr.ref_wide(rh, roff, xh, xoff, triangle, metric, 20, max_dist, want_dense=True)
        qr.assert_same_hits(wide, want, "ref_wide")
        assert np.array_equal(wd, wdense)


def test_model_counts_repeats_on_both_sides():
    # query hash 5 twice, reference 0 lists hash 5 twice: 2 x 2 = 4 (src/dist.cpp:199-202 runs the inner loop per occurrence)
    rh, roff = qr.csr([[5, 5, 9], [5, 7]])
    qh, qoff = qr.csr([[5, 5, 7]])
    _, dense = qr.numpy_model(rh, roff, qh, qoff, 0, 0, 20, 1.5, want_dense=True)
    assert dense.tolist() == [[4, 3]]
    postings, counts = ok.index_build32(rh, roff, 8)
    _, wdense = ok.index_dist32(counts, 8, postings, np.diff(roff).astype(np.uint32), qh, qoff, 0, 0, 20, 1.5, want_dense=True)
    assert wdense.tolist() == [[4, 3]]
