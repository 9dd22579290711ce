"""tests/_topn_ref.py, the reference of tests/test_gpu_topn_edges.py, checked without a GPU: its records give the text of the real
reference's `dist -N` outputs (tests/golden/dist), its distances are the oracle's bit for bit (the C library's log), its builder
yields exactly the prescribed cells, and its shard rows are those of tests/_gather_ref.py."""
import json
import os
import re

import numpy as np

import _gather_ref as ga
import _topn_ref as tr
from conftest import GOLDEN, ROOT
from oracle import oracle as ok
from rabbitkssd_amd import capi


def test_reference_gives_the_golden_dist_n_files():
    d = os.path.join(GOLDEN, "dist")
    man = json.load(open(os.path.join(d, "manifest.json")))
    _, rnames, rh, roff = ok.read_sketches32(os.path.join(d, "ref.sketch"))
    _, qnames, qh, qoff = ok.read_sketches32(os.path.join(d, "qry.sketch"))
    refs = [np.unique(p) for p in ga.parts_of(rh, roff)]
    queries = [np.unique(p) for p in ga.parts_of(qh, qoff)]
    assert [len(p) for p in refs] == np.diff(roff).tolist() and [len(p) for p in queries] == np.diff(qoff).tolist()   # sets
    cell = tr.cells(refs, queries)
    k = 2 * man["half_k"]
    n_cases = 0
    for case in man["cases"]:
        if case["cmd"] != "dist" or not case["max_neighbor"]:
            continue
        want = open(os.path.join(d, case["file"])).read().split("\n")[:-1]
        mine = tr.reference(cell, case["metric"], k, case["max_dist"], case["max_neighbor"])
        assert [capi.format_hit(qnames[h["row"]], rnames[h["col"]], h).rstrip("\n") for h in mine] == want, case["file"]
        n_cases += 1
    assert n_cases >= 12     # M0/M1 x D {0.1, 1} x N {1, 3, 100}


def test_distances_are_the_oracles_bit_for_bit():
    rng = np.random.default_rng(5)
    size0 = rng.integers(0, 501, size=4000)
    size1 = rng.integers(0, 501, size=4000)
    common = (np.minimum(size0, size1) * rng.random(4000) ** 2).astype(np.int64)
    size0[:50] = size1[:50] = rng.integers(1, 501, size=50)
    common[:50] = size0[:50]                             # identical sets: jorc 1.0, distance 0.0
    for metric in (0, 1):
        for k in (1, 2, 3, 5, 20):
            j, d = tr.distances(common, size0, size1, metric, k)
            want = np.array([ok.distance(int(c), int(a), int(b), metric, k) for c, a, b in zip(common, size0, size1)])
            assert j.tobytes() == want[:, 0].tobytes() and d.tobytes() == want[:, 1].tobytes(), (metric, k)
            assert (d == 1.0).any() and (d == 0.0).any() and ((d > 1.0).any() or k == 20)


def test_builder_yields_the_prescribed_cells():
    for bits, seed in ((22, 1), (24, 2), (36, 3)):
        rng = np.random.default_rng(seed)
        pool = tr.Pool(bits, seed)
        queries = [np.sort(pool.take(n)) for n in (300, 40, 0, 500)]
        R = 120
        sizes = rng.integers(0, 501, size=R)
        sizes[0] = 0
        common = np.zeros((4, R), dtype=np.int64)
        for j in range(R):
            left = int(sizes[j])
            for q in rng.permutation(4):
                common[q, j] = rng.integers(0, min(left, len(queries[q])) + 1) if rng.random() < 0.7 else 0
                left -= common[q, j]
        refs = tr.build_refs(pool, rng, queries, common, sizes)
        everything = np.concatenate(queries + refs)
        assert int(everything.max()) < 1 << bits and (bits < 36 or int(everything.max()) >= 1 << 32)
        got_common, size0, size1 = tr.cells(refs, queries)
        assert np.array_equal(got_common, common) and np.array_equal(size0, sizes) and size1.tolist() == [300, 40, 0, 500]
        assert all(len(np.unique(r)) == len(r) for r in refs)
        # private hashes are private: a hash held by two sketches is one of a query's
        h, n = np.unique(everything, return_counts=True)
        assert np.isin(h[n > 1], np.concatenate(queries)).all()
        # not a prefix: some reference takes a hash beyond the first common[q][j] of its query
        assert any(common[0, j] and not np.isin(refs[j], queries[0][:common[0, j]]).sum() == common[0, j] for j in range(R))


def test_shard_rows_are_the_block_cyclic_rows():
    for n in (0, 1, 22, 23):
        for first, step, block in ((0, 1, 0), (0, 3, 4), (1, 3, 4), (2, 3, 4), (7, 9, 4), (1, 2, 1)):
            assert tr.shard_rows(n, first, step, block) == ga.selected_rows(n, first, step, block)
    assert tr.shard_rows(23, 2, 3, 4) == [8, 9, 10, 11, 20, 21, 22] and tr.shard_rows(23, 7, 9, 4) == []


def test_stage_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    for name in ("COUNTS", "SELECT", "DOWNLOAD", "HOST", "CANDIDATES"):
        assert int(re.search(r"#define RK_MS_TOPN_%s (\d+)\b" % name, hdr).group(1)) == getattr(capi, "MS_TOPN_" + name)
