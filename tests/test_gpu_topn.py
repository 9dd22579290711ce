"""`dist -N` on the device (rk_dist_topn, GPU): record for record, bit for bit, what rk_dist_rows + rk_topn_rows return on the
same inputs, and what the oracle's index_dist + heap return -- on the golden fixtures, on orders built against the selection
kernel, on a renumbered index, in several batches with a candidate overflow, on 64-bit hashes, at BASELINE configs[4], and
through the command-line tool."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth

pytestmark = pytest.mark.gpu
CORES = max(1, len(os.sched_getaffinity(0)))
TOOL = os.path.join(ROOT, "rabbitkssd_amd", "rabbit_kssd")


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def old_path(ctx, idx, qs, metric, k, D, N, **kw):
    hits, _ = ctx.dist_rows(idx, qs, 0, metric, k, D, **kw)
    return capi.topn_rows(hits, N)


def assert_same(mine, want):
    assert len(mine) == len(want)
    assert mine.tobytes() == want.tobytes()     # row, col, common, sizes, jorc and dist bit for bit, same order


def oracle_topn(rh, roff, bits, qh, qoff, rows, metric, k, D, N):
    """the oracle's index_dist on the listed query rows + its heap, rows renumbered back"""
    postings, counts = ok.index_build32(rh, roff, bits)
    rows = np.asarray(rows)
    parts = [qh[int(qoff[q]):int(qoff[q + 1])] for q in rows]
    s_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    s_h = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
    hits, _ = ok.index_dist32(counts, bits, postings, np.diff(roff).astype(np.uint32), s_h, s_off, 0, metric, k, D,
                              threads=CORES)
    out = []
    for i, q in enumerate(rows):
        t = ok.topn_row(hits[hits["row"] == i], N).copy()
        t["row"] = q
        out.append(t)
    return np.concatenate(out)


def assert_oracle(mine, want):
    sel = mine[np.isin(mine["row"], np.unique(want["row"]))]
    assert len(sel) == len(want)
    for f in ("row", "col", "common", "size0", "size1", "jorc", "dist"):
        assert np.array_equal(sel[f], want[f]), f


def csr(sets):
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.uint64)
    h = np.concatenate([np.asarray(s, dtype=np.uint32) for s in sets]) if sets else np.zeros(0, np.uint32)
    return h, off


def test_triangle_is_refused(ctx):
    _, h, off = synth.clade_sketches(20, 50, 20)
    idx = ctx.index_build(ctx.sketches_from_host(h, off), 20)
    qs = ctx.sketches_from_host(h, off)
    with pytest.raises(capi.RkError) as e:
        ctx.dist_topn(idx, qs, 0, 20, 1.0, 3, triangle=1)
    assert e.value.code == -1
    assert len(ctx.dist_topn(idx, qs, 0, 20, 1.0, 0)) == 0          # N = 0: nothing, as rk_topn_rows keeps


def test_golden_fixtures(ctx):
    d = os.path.join(GOLDEN, "dist")
    man = json.load(open(os.path.join(d, "manifest.json")))
    _, rnames, rh, roff = ok.read_sketches32(os.path.join(d, "ref.sketch"))
    _, qnames, qh, qoff = ok.read_sketches32(os.path.join(d, "qry.sketch"))
    k = 2 * man["half_k"]
    qs = ctx.sketches_from_host(qh, qoff)
    built = ctx.index_build(ctx.sketches_from_host(rh, roff), man["hash_bits"])
    postings, counts = ok.index_build32(rh, roff, man["hash_bits"])
    imported = ctx.index_import(postings, counts, man["hash_bits"], np.diff(roff))
    n_cases = 0
    for case in man["cases"]:
        if case["cmd"] != "dist" or not case["max_neighbor"]:
            continue
        want = open(os.path.join(d, case["file"])).read().split("\n")[:-1]
        for idx in (built, imported):
            mine = ctx.dist_topn(idx, qs, case["metric"], k, case["max_dist"], case["max_neighbor"])
            assert_same(mine, old_path(ctx, idx, qs, case["metric"], k, case["max_dist"], case["max_neighbor"]))
            text = [capi.format_hit(qnames[h["row"]], rnames[h["col"]], h).rstrip("\n") for h in mine]
            assert text == want, case["file"]
        n_cases += 1
    assert n_cases >= 12     # M0/M1 x D {0.1, 1} x N {1, 3, 100}


def test_nested_references_every_cell_a_candidate(ctx):
    """Reference j is the first 5 + 3j hashes of the query: the distance falls with the column, every cell beats the heap
    top, the candidates of a row are all R cells -- more than the first capacity (1024 + 16 N per row): the retry runs."""
    rng = np.random.default_rng(1)
    q = np.sort(rng.choice(1 << 22, size=8000, replace=False)).astype(np.uint32)
    R = 2500
    refs = [q[:5 + 3 * j] for j in range(R)]
    rh, roff = csr(refs)
    qh, qoff = csr([q, q[:4000], q[::2]])
    idx = ctx.index_build(ctx.sketches_from_host(rh, roff), 22)
    qs = ctx.sketches_from_host(qh, qoff)
    for metric in (0, 1):
        for N in (1, 5, 100):
            mine = ctx.dist_topn(idx, qs, metric, 20, 1.0, N)
            assert_same(mine, old_path(ctx, idx, qs, metric, 20, 1.0, N))
    assert_oracle(mine, oracle_topn(rh, roff, 22, qh, qoff, [0, 1, 2], 1, 20, 1.0, 100))


def test_duplicates_unrelated_queries_and_empty_sketches(ctx):
    """60 copies of one reference sketch (interior ties, N below the copies), unrelated queries at -D 1.0 (every cell 1.0),
    an empty reference and an empty query."""
    rng = np.random.default_rng(2)
    bits = 24
    base = np.sort(rng.choice(1 << bits, size=300, replace=False)).astype(np.uint32)
    refs = []
    for j in range(3000):
        if j % 50 == 7:
            refs.append(base)                               # the duplicates, spread over the columns
        elif j == 1234:
            refs.append(np.zeros(0, np.uint32))             # an empty reference
        else:
            refs.append(np.sort(rng.choice(1 << bits, size=int(rng.integers(50, 400)), replace=False)).astype(np.uint32))
    rh, roff = csr(refs)
    related = np.union1d(base[:200], rng.choice(1 << bits, size=3000, replace=False)).astype(np.uint32)
    unrelated = np.sort(rng.choice(1 << bits, size=2000, replace=False)).astype(np.uint32)
    qh, qoff = csr([related, unrelated, np.zeros(0, np.uint32), related[::3]])
    idx = ctx.index_build(ctx.sketches_from_host(rh, roff), bits)
    qs = ctx.sketches_from_host(qh, qoff)
    for metric in (0, 1):
        for D in (1.0, 2.0):
            for N in (1, 3, 20, 1024):
                mine = ctx.dist_topn(idx, qs, metric, 20, D, N)
                assert_same(mine, old_path(ctx, idx, qs, metric, 20, D, N))
    assert_oracle(mine, oracle_topn(rh, roff, bits, qh, qoff, [0, 1, 2, 3], 1, 20, 2.0, 1024))
    # the empty query: N references at exactly 1.0, the first N columns in the reference heap's pop order
    e = ctx.dist_topn(idx, qs, 0, 20, 1.0, 3)
    e = e[e["row"] == 2]
    assert len(e) == 3 and set(e["dist"]) == {1.0}


def test_relabeled_index_and_block_cyclic_shards(ctx):
    """Clades listed in shuffled order: the index renumbers them (rk_index_order is not the identity), counter rows leave
    the device in the caller's column order, the sizes are gathered to it.  Row shards equal the whole."""
    names, h, off = synth.clade_sketches(4000, 120, 24, seed=9)
    names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(4000, "shuffled"))
    idx = ctx.index_build(ctx.sketches_from_host(h, off), 24)
    assert not np.array_equal(idx.order, np.arange(4000))
    rows = np.arange(0, 4000, 37)
    qh, qoff = csr([h[int(off[r]):int(off[r + 1])] for r in rows])
    qs = ctx.sketches_from_host(qh, qoff)
    for metric in (0, 1):
        for N in (1, 10):
            mine = ctx.dist_topn(idx, qs, metric, 20, 1.0, N)
            assert_same(mine, old_path(ctx, idx, qs, metric, 20, 1.0, N))
    assert_oracle(mine, oracle_topn(h, off, 24, qh, qoff, np.arange(0, len(rows), 9), 1, 20, 1.0, 10))
    parts = [ctx.dist_topn(idx, qs, 0, 20, 1.0, 10, row_first=r, row_step=3, row_block=4) for r in range(3)]
    merged = np.concatenate(parts)
    merged = merged[np.argsort(merged["row"], kind="stable")]
    assert_same(merged, ctx.dist_topn(idx, qs, 0, 20, 1.0, 10))
    for r in range(3):
        assert_same(parts[r], old_path(ctx, idx, qs, 0, 20, 1.0, 10, row_first=r, row_step=3, row_block=4))


def test_batches_and_candidate_overflow(monkeypatch):
    """RK_TOPN_BATCH_BYTES of two counter rows (11 queries: 6 batches) and RK_TOPN_CAND_CAP of 16 records (every batch
    overflows and runs its selection again with the exact count)."""
    names, h, off = synth.clade_sketches(3000, 150, 24, seed=12)
    rows = np.arange(5, 3000, 271)
    qh, qoff = csr([h[int(off[r]):int(off[r + 1])] for r in rows])
    plain = capi.Context(0)
    want = {}
    for metric in (0, 1):
        idx = plain.index_build(plain.sketches_from_host(h, off), 24)
        want[metric] = old_path(plain, idx, plain.sketches_from_host(qh, qoff), metric, 20, 1.0, 7)
    monkeypatch.setenv("RK_TOPN_BATCH_BYTES", str(2 * 3000 * 4))
    monkeypatch.setenv("RK_TOPN_CAND_CAP", "16")
    small = capi.Context(0)
    idx = small.index_build(small.sketches_from_host(h, off), 24)
    qs = small.sketches_from_host(qh, qoff)
    for metric in (0, 1):
        assert_same(small.dist_topn(idx, qs, metric, 20, 1.0, 7), want[metric])
    steady = small.pool_stats()
    small.dist_topn(idx, qs, 0, 20, 1.0, 7)
    assert small.pool_stats()[2:] == steady[2:]        # steady state: no new device allocation
    monkeypatch.setenv("RK_DIST_TOPN", "0")
    ab = capi.Context(0)
    idx = ab.index_build(ab.sketches_from_host(h, off), 24)
    assert_same(ab.dist_topn(idx, ab.sketches_from_host(qh, qoff), 1, 20, 1.0, 7), want[1])


def test_small_collection_many_queries_large_n_stays_in_budget(monkeypatch):
    """1,000 references, 6,000 queries, -N 500 and 1024 (> R): a row can emit no more than its 1,000 cells, so the candidate
    room per row is min(R, 1024 + 16 N) and the counter rows + candidate buffers of a batch fit RK_TOPN_BATCH_BYTES -- the
    default 1 GiB, and 64 MB (14 batches, also with the sliced membership pass, which runs with the first batch only).  What
    the calls add to the context's pool stays within twice the budget: the pool keeps the blocks of a batch cached, and the
    radix sort's scratch of a smaller last batch may come as a block of its own (one batch alone, at the default budget, stays
    within 1.1 x).  Sized by Q x (1024 + 16 N) instead, the candidates alone would take 2.6 GB at -N 500."""
    names, rh, roff = synth.clade_sketches(1000, 100, 24, seed=41)
    qh, qoff = csr([rh[int(roff[r]):int(roff[r + 1])] for r in range(1000)] * 6)
    plain = capi.Context(0)
    idx = plain.index_build(plain.sketches_from_host(rh, roff), 24)
    want = {N: old_path(plain, idx, plain.sketches_from_host(qh, qoff), 0, 20, 1.0, N) for N in (500, 1024)}
    assert len(want[500]) == 6000 * 500 and len(want[1024]) == 6000 * 1000
    plain.close()
    for budget, sliced in ((None, False), (64 << 20, False), (64 << 20, True)):
        if budget:
            monkeypatch.setenv("RK_TOPN_BATCH_BYTES", str(budget))
        if sliced:
            monkeypatch.setenv("RK_DISTQ_SLICED", "1")
        c = capi.Context(0)
        idx = c.index_build(c.sketches_from_host(rh, roff), 24)
        qs = c.sketches_from_host(qh, qoff)
        c.trim()
        live = c.pool_stats()[0]
        for N in (500, 1024):
            assert_same(c.dist_topn(idx, qs, 0, 20, 1.0, N), want[N])
        added = c.pool_stats()[0] - live
        assert added <= (2 * budget if budget else 1.1 * (1 << 30)) + (16 << 20), (budget, added)
        c.close()


def test_wide_hashes_and_sparse_thresholds(ctx):
    """64-bit hashes (rk_sketches_from_host64), both metrics; a threshold that excludes 1.0 takes the plain path inside."""
    names, h, off = synth.clade_sketches(1500, 200, 36, seed=14, wide=True)
    rows = np.arange(3, 1500, 97)
    parts = [h[int(off[r]):int(off[r + 1])] for r in rows]
    qoff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    qh = np.concatenate(parts)
    idx = ctx.index_build(ctx.sketches_from_host64(h, off), 36)
    qs = ctx.sketches_from_host64(qh, qoff)
    for metric in (0, 1):
        for D, N in ((1.0, 1), (1.0, 12), (0.2, 4)):
            assert_same(ctx.dist_topn(idx, qs, metric, 20, D, N), old_path(ctx, idx, qs, metric, 20, D, N))


def test_config4_full_size():
    """BASELINE configs[4] with -N 5 -D 1.0: 100,000 references of 76 hashes x 1,000 queries of ~45,776 (24-bit).  50 queries
    with planted references equal the oracle; 5,000 records.  Device memory: the call itself takes at most 0.6 GB of the
    context's pool (one batch of 1,000 counter rows of 100,000 int32 is 0.4 GB, the candidates ~0.03 GB) and the whole
    context -- index and the 183 MB of query hashes included -- stays below 1.5 GB, where the plain path holds 10^8 records of
    40 B (4 GB) before the sort's buffers."""
    rn, rh, roff = synth.clade_sketches(100000, 76, 24, seed=31)
    qn, qh, qoff = synth.clade_sketches(1000, 45776, 24, seed=32)
    rng = np.random.default_rng(4)
    sample = np.sort(rng.choice(1000, size=50, replace=False))
    parts = [qh[int(qoff[q]):int(qoff[q + 1])] for q in range(1000)]
    for q in sample:
        refs = rng.choice(100000, size=5, replace=False)
        parts[q] = np.unique(np.concatenate([parts[q]] + [rh[int(roff[r]):int(roff[r + 1])] for r in refs]))
    qh, qoff = csr(parts)
    fresh = capi.Context(0)
    idx = fresh.index_build(fresh.sketches_from_host(rh, roff), 24)
    qs = fresh.sketches_from_host(qh, qoff)
    fresh.trim()                      # (the build's and the upload's temporaries back to the driver: what remains is live)
    live = fresh.pool_stats()[0]
    mine = fresh.dist_topn(idx, qs, 0, 20, 1.0, 5)
    peak = fresh.pool_stats()[0]
    assert len(mine) == 5000 and np.array_equal(np.unique(mine["row"]), np.arange(1000))
    assert peak - live <= 0.6e9 and peak <= 1.5e9, (live, peak)
    assert_oracle(mine, oracle_topn(rh, roff, 24, qh, qoff, sample, 0, 20, 1.0, 5))
    # containment on the same objects, against the oracle again
    mine = fresh.dist_topn(idx, qs, 1, 20, 1.0, 5)
    assert_oracle(mine, oracle_topn(rh, roff, 24, qh, qoff, sample[:10], 1, 20, 1.0, 5))


def run_tool(args, cwd, env=None):
    p = subprocess.run([TOOL] + [str(a) for a in args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **(env or {})), timeout=300)
    assert p.returncode == 0, p.stderr.decode()


def test_cli_dist_minus_n(tmp_path):
    """`rabbit_kssd dist -N 5` on .sketch files: the text of the device path equals the text of RK_DIST_TOPN=0, with one GPU
    and with two query blocks (--gpus 2: a second card, or --same-device on one)."""
    names, h, off = synth.clade_sketches(2500, 150, 24, seed=21)
    synth.write_sketch_file(str(tmp_path / "ref.sketch"), 10, 6, 4, names, h, off)
    rows = np.arange(1, 2500, 41)
    qh, qoff = csr([h[int(off[r]):int(off[r + 1])] for r in rows])
    synth.write_sketch_file(str(tmp_path / "qry.sketch"), 10, 6, 4, ["q%d" % r for r in rows], qh, qoff)
    two = ["--gpus", 2] + ([] if capi.lib().rk_device_count() >= 2 else ["--same-device"])
    for metric in (0, 1):
        for extra in ([], ["--gpus", 1], two):
            args = ["dist", "-r", "ref.sketch", "-q", "qry.sketch", "-N", 5, "-M", metric] + extra
            run_tool(args + ["-o", "new.txt"], tmp_path)
            run_tool(args + ["-o", "old.txt"], tmp_path, env={"RK_DIST_TOPN": "0"})
            new, old = (tmp_path / "new.txt").read_bytes(), (tmp_path / "old.txt").read_bytes()
            assert new == old and new.count(b"\n") >= 5 * len(rows), (metric, extra)
