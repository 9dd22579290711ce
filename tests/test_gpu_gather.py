"""rk_gather_rows on the device against tests/_gather_ref.py: the real reference's intersection counts on the golden pairs, random
collections under every option and both hash widths, greedy against rank-by-overlap, ties under every caller order, the walks of the
cover kernel at their seams (read from the call's stats, not copied), many rounds, many candidates, batches, row shards, the empty
cases, the host leg, the round trip from rk_group_sketches, the refusals and `rabbit_kssd gather`.  Every case asserts from the stats
which leg ran, how many rounds it took and how many batches ran, then compares every output array exactly."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _gather_ref as ga
from _selfjoin_cases import TOOL, csr, device_index
from conftest import GOLDEN
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth
from test_gather_cpu import OPTIONS, ROWS_ARGTYPES
from test_gpu_group import imported_index, index_of

pytestmark = pytest.mark.gpu
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def queries_of(ctx, parts, wide=False):
    h, off = csr(parts, np.uint64 if wide else np.uint32)
    return ctx.sketches_from_host64(h, off) if wide else ctx.sketches_from_host(h, off)


def launched_rounds(result, rows, refs, queries, max_picks, sync_every, rows_per_batch):
    """the rounds the host launches: per batch, up to the first read of the live-row counter at or after the round in which the last
    row retires -- a row retires with its last pick when that leaves nothing or reaches max_picks, else in the round after"""
    total = 0
    for b in range(0, len(rows), rows_per_batch):
        need, biggest = 0, 0
        for q in rows[b:b + rows_per_batch]:
            picks = result[q][0]
            at_pick = picks and (picks[-1][5] == 0 or len(picks) == max_picks)
            need = max(need, len(picks) if at_pick else len(picks) + 1)
            biggest = max(biggest, len(set(int(h) for h in queries[q])))
        last = min(max_picks if max_picks else 1 << 32, biggest, len(refs)) + 1   # the last round the host can launch
        total += min(-(-need // sync_every) * sync_every, last)
    return total


def gathered(ctx, idx, qs, refs, queries, min_new=1, max_picks=0, path=1, want=None, **rows):
    """the call, with what every result must satisfy, compared exactly with the reference; returns (arrays, stats)"""
    got = ctx.gather_rows(idx, qs, min_new, max_picks, **rows)
    off, picks, matched, n_cand, covered, st = got
    sel = ga.selected_rows(len(queries), rows.get("row_first", 0), rows.get("row_step", 1), rows.get("row_block", 0))
    result = want if want is not None else ga.fast(refs, queries, min_new, max_picks)
    w_off, w_picks, w_matched, w_cand, w_covered = ga.as_arrays(result, refs, queries, sel)
    assert st["path"] == path and st["rows"] == len(sel)
    assert off.tolist() == w_off and ga.pick_tuples(picks) == w_picks
    assert matched.tolist() == w_matched and n_cand.tolist() == w_cand and covered.tolist() == w_covered
    assert st["picks"] == len(w_picks) and st["matched"] == sum(w_matched) and st["candidates"] == sum(w_cand)
    assert st["rounds"] == max([len(result[q][0]) for q in sel] + [0])
    assert st["lane_max"] >= 1 and st["wave_max"] >= st["lane_max"] and st["sync_every"] >= 1 and st["threads"] >= 64
    if not len(sel) or not len(refs):
        assert st["batches"] == 0 and st["launches"] == 0 and st["launched_rounds"] == 0
    elif path == 1:
        assert 1 <= st["rows_per_batch"] <= len(sel) and st["batches"] == -(-len(sel) // st["rows_per_batch"])
        assert st["launched_rounds"] == launched_rounds(result, sel, refs, queries, max_picks, st["sync_every"], st["rows_per_batch"])
        assert st["read_backs"] >= 2 * st["batches"] and st["launches"] >= st["launched_rounds"] + 4 * st["batches"]
        died = st["lane_lists"] + st["wave_lists"] + st["block_lists"]
        assert died <= st["matched"] and st["decrements"] >= died
    else:
        assert st["batches"] == 1 and st["launches"] == 0 and st["launched_rounds"] == 0 and st["decrements"] == 0
    if min_new == 1 and not max_picks:
        assert covered.tolist() == matched.tolist()
    return got[:5], st


def result_bytes(arrays):
    return b"".join(a.tobytes() for a in arrays)


# ---- 1. the real reference's intersection counts ------------------------------------------------------------------------------------
def golden_pair(tag):
    read = ok.read_sketches64 if tag == "64" else ok.read_sketches32
    d, s = ("dist64", "64") if tag == "64" else ("dist", "")
    _, rnames, rh, roff = read(os.path.join(GOLDEN, d, "ref%s.sketch" % s))
    _, qnames, qh, qoff = read(os.path.join(GOLDEN, d, "qry%s.sketch" % s))
    triples = {}
    for line in open(os.path.join(GOLDEN, d, "dist%s_M0_D1_N0.ref.txt" % s)):
        f = line.rstrip("\n").split("\t")
        triples[(f[0], f[1])] = tuple(int(x) for x in f[2].split("|"))
    return rnames, ga.parts_of(rh, roff), qnames, ga.parts_of(qh, qoff), triples


@pytest.mark.parametrize("tag,how", [("32", "built"), ("32", "imported"), ("64", "built"), ("64", "imported")])
def test_golden_pairs_carry_the_references_own_counts(ctx, tag, how):
    rnames, refs, qnames, queries, triples = golden_pair(tag)
    wide, bits = (True, 36) if tag == "64" else (False, 24)
    assert len(triples) == len(refs) * len(queries)
    idx = (index_of if how == "built" else imported_index)(ctx, refs, wide, bits)
    qs = queries_of(ctx, queries, wide)
    for min_new, max_picks in ((1, 0), (5, 3)):
        (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, qs, refs, queries, min_new, max_picks)
        assert st["batches"] == 1 and len(picks) >= 1
        for p in picks:   # the real reference's intersection count and sizes of that pair
            assert (int(p["common"]), int(p["size_ref"]), int(p["size_query"])) == triples[(qnames[p["query"]], rnames[p["ref"]])]
        for q in range(len(queries)):
            assert n_cand[q] == sum(triples[(qnames[q], r)][0] >= min_new for r in rnames)


# ---- 2. random collections, every option, both widths ---------------------------------------------------------------------------------
_clades = {}


def clades(wide):
    """(refs, queries, bits): 1,000 genomes in clades of 10, sketches of about 40 hashes, in a shuffled caller order; 40 queries that
    are unions of 1 .. 6 genomes plus foreign hashes, one empty query and one of foreign hashes only"""
    if wide not in _clades:
        bits, kmer = (36, 24) if wide else (24, 20)
        names, h, off = synth.clade_sketches(1000, 40, bits, kmer_size=kmer, strains_per_clade=10, seed=91 + wide, wide=wide)
        names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(len(names), "shuffled", seed=6))
        refs = ga.parts_of(h, off)
        rng = np.random.default_rng(17 + wide)
        dtype = np.uint64 if wide else np.uint32
        queries = []
        for k in range(40):
            members = rng.choice(len(refs), size=1 + k % 6, replace=False)
            if k % 3 == 0:   # relatives: strains of one clade explain each other's hashes
                members = np.concatenate([members, [int(np.argmax([len(np.intersect1d(refs[members[0]], r)) if i != members[0] else 0 for i, r in enumerate(refs)]))]])
            foreign = rng.integers(0, 1 << bits, size=int(rng.integers(0, 30)), dtype=np.uint64)
            queries.append(np.unique(np.concatenate([refs[m].astype(np.uint64) for m in members] + [foreign])).astype(dtype))
        indexed = np.unique(h)
        queries.append(np.zeros(0, dtype=dtype))
        queries.append(np.setdiff1d(rng.integers(0, 1 << bits, size=50, dtype=np.uint64), indexed.astype(np.uint64)).astype(dtype))
        _clades[wide] = (refs, queries, bits)
    return _clades[wide]


_wanted = {}


def wanted(wide, min_new, max_picks):
    """the reference's answer on clades(wide), computed once and shared"""
    key = (wide, min_new, max_picks)
    if key not in _wanted:
        refs, queries, bits = clades(wide)
        _wanted[key] = ga.fast(refs, queries, min_new, max_picks)
    return _wanted[key]


@pytest.mark.parametrize("wide", [False, True])
def test_random_collections_under_every_option(ctx, wide):
    refs, queries, bits = clades(wide)
    idx = index_of(ctx, refs, wide, bits)
    order = idx.order
    assert not np.array_equal(order, np.arange(len(refs)))   # internal order != caller order
    qs = queries_of(ctx, queries, wide)
    before = ctx.dist_rows(idx, qs, 0, 0, 20, 0.3)[0]
    for min_new, max_picks in OPTIONS:
        want = wanted(wide, min_new, max_picks)
        arrays, st = gathered(ctx, idx, qs, refs, queries, min_new, max_picks, want=want)
        assert st["batches"] == 1
        if (min_new, max_picks) == (1, 0):
            ga.singled_out(refs, queries, want)
            assert st["rounds"] >= 5 and sum(len(r[0]) > 3 for r in want) > 10   # many queries take several rounds
            lists = ga.posting_lists(refs)
            assert 0 < st["decrements"] <= sum(len(lists.get(h, ())) for q in queries for h in q.tolist())   # a list dies at most once
    after = ctx.dist_rows(idx, qs, 0, 0, 20, 0.3)[0]
    assert len(before) > 40 and before.tobytes() == after.tobytes()   # index and queries are unchanged by the calls


def test_built_and_imported_indexes_give_the_same_bytes(ctx):
    refs, queries, bits = clades(True)
    qs = queries_of(ctx, queries, True)
    a, _ = gathered(ctx, index_of(ctx, refs, True, bits), qs, refs, queries, want=wanted(True, 1, 0))
    b, _ = gathered(ctx, imported_index(ctx, refs, True, bits), qs, refs, queries, want=wanted(True, 1, 0))
    assert result_bytes(a) == result_bytes(b)


# ---- 3. greedy is not rank-by-overlap ---------------------------------------------------------------------------------------------------
def test_greedy_is_not_rank_by_overlap(ctx):
    """A holds most of the query, B lies almost inside A, C is small and disjoint: by overlap A B C, greedily A C B -- and B is dropped
    at min_new = 2.  Without the decrements B would come second with fresh 30."""
    pool = np.random.default_rng(3).permutation(1 << 22)[:200].astype(np.uint32)
    A, B, C_ = np.sort(pool[:60]), np.sort(pool[29:61]), np.sort(pool[100:110])   # B: 31 of A's hashes and one of its own
    query = np.sort(np.concatenate([pool[:61], pool[100:110], pool[150:160]]))
    for order in itertools.permutations(range(3)):
        refs = [None] * 3
        for role, at in zip((A, B, C_), order):
            refs[at] = role
        a, b, c = order
        idx, qs = index_of(ctx, refs), queries_of(ctx, [query])
        (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, qs, refs, [query])
        assert [(p["ref"], p["common"], p["fresh"], p["left"]) for p in picks] == [(a, 60, 60, 11), (c, 10, 10, 1), (b, 32, 1, 0)]
        assert matched.tolist() == [71] and st["rounds"] == 3
        (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, qs, refs, [query], min_new=2)
        assert [int(p["ref"]) for p in picks] == [a, c] and covered.tolist() == [70] and n_cand.tolist() == [3]


# ---- 4. ties ----------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smaller_caller_index_under_every_order(ctx):
    pool = np.random.default_rng(4).permutation(1 << 22)[:400].astype(np.uint32)
    X, Y, Z = np.sort(pool[0:40]), np.sort(pool[40:80]), np.sort(pool[80:120])
    # equal only after a decrement: U holds 50, V 45 of which 10 are U's, W 35 disjoint: after U, V and W both have 35
    U, V, W = np.sort(pool[200:250]), np.sort(pool[240:285]), np.sort(pool[300:335])
    cases = ((X, Y, Z, np.sort(pool[0:120])),                    # three equal in round 0
             (X, Y, np.sort(pool[80:110]), np.sort(pool[0:120])),   # two equal in round 0, a smaller third
             (U, V, W, np.sort(pool[200:335])))
    for n_case, (r0, r1, r2, query) in enumerate(cases):
        for order in itertools.permutations(range(3)):   # role k sits at caller index order[k]: internal order != caller order
            refs = [None] * 3
            for role, at in zip((r0, r1, r2), order):
                refs[at] = role
            extra = [np.sort(pool[350 + 5 * k: 355 + 5 * k]) for k in range(3)]   # bystanders, so that the build has something to renumber
            refs = refs + extra
            (off, picks, matched, n_cand, covered), st = gathered(ctx, index_of(ctx, refs), queries_of(ctx, [query]), refs, [query])
            got = [(int(p["ref"]), int(p["fresh"])) for p in picks]
            if n_case == 0:
                assert got == [(0, 40), (1, 40), (2, 40)]
            elif n_case == 1:
                assert got == sorted([(order[0], 40), (order[1], 40)]) + [(order[2], 30)]
            else:
                assert got == [(order[0], 50)] + sorted([(order[1], 35), (order[2], 35)])


# ---- 5. lists at the seams of the cover walk ----------------------------------------------------------------------------------------------
def constants(ctx):
    one = [np.array([1], dtype=np.uint32)]
    st = ctx.gather_rows(index_of(ctx, one), queries_of(ctx, one))[5]
    return st["lane_max"], st["wave_max"], st["threads"]


def test_identical_references_one_pick_one_round(ctx):
    one = np.unique(np.random.default_rng(8).integers(0, 1 << 24, size=130))[:100].astype(np.uint32)
    refs = [one] * 300
    (off, picks, matched, n_cand, covered), st = gathered(ctx, index_of(ctx, refs), queries_of(ctx, [one]), refs, [one])
    assert ga.pick_tuples(picks) == [(0, 0, 0, 100, 100, 0, 100, 100)] and n_cand.tolist() == [300] and st["rounds"] == 1
    # the row retires with its pick: nothing is left, no list is walked
    assert st["decrements"] == 0 and st["lane_lists"] + st["wave_lists"] + st["block_lists"] == 0
    # a second query keeps the batch going: its rounds do not disturb the retired row
    two = [one, np.unique(np.concatenate([one[:50], [1 << 23]])).astype(np.uint32)]
    gathered(ctx, index_of(ctx, refs), queries_of(ctx, two), refs, two)


N_SEAM = 700


def test_every_walk_of_the_cover_kernel_at_its_seams(ctx, monkeypatch):
    lane_max, wave_max, threads = constants(ctx)
    assert 1 <= lane_max < wave_max and 2 * threads + 1 < N_SEAM
    # a = the first length a walk does NOT take; 64 and 65: one trip of a wave and the next
    lengths = sorted({1, 2, N_SEAM} | {a + d for a in (lane_max + 1, wave_max + 1, 65, threads + 1, 2 * threads + 1) for d in (-1, 0, 1)})
    rng = np.random.default_rng(12)
    pool = rng.permutation(1 << 22)[: 4 * N_SEAM + len(lengths)].astype(np.uint32)
    parts = [list(pool[4 * v: 4 * v + 4]) for v in range(N_SEAM)]
    shared = pool[4 * N_SEAM:]
    hub, second = 17, 400
    for L, s in zip(lengths, shared):   # the hub holds every shared hash, L - 1 others hold it with the hub
        others = rng.choice([v for v in range(N_SEAM) if v not in (hub, second)], size=L - 1, replace=False) if L < N_SEAM else [v for v in range(N_SEAM) if v != hub]
        for v in [hub] + list(others):
            parts[v].append(s)
    refs = [np.sort(np.array(p, dtype=np.uint32)) for p in parts]
    # the query: every shared hash, and three private hashes of `second`, which keep the row alive past the hub's round
    query = np.sort(np.concatenate([shared, np.array(parts[second][:3], dtype=np.uint32)]))
    idx, qs = index_of(ctx, refs), queries_of(ctx, [query])
    assert idx.distinct == 4 * N_SEAM + len(lengths)
    want = ga.fast(refs, [query])
    assert [p[1] for p in want[0][0]][:1] == [hub] and want[0][0][0][4] == len(lengths)   # round 0 kills every shared list
    for split in (True, False):
        if not split:
            monkeypatch.setenv("RK_GATHER_SPLIT", "0")
        (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, qs, refs, [query], want=want)
        if split:
            assert (st["lane_max"], st["wave_max"]) == (lane_max, wave_max)
            assert st["lane_lists"] == sum(L <= lane_max for L in lengths)
            assert st["wave_lists"] == sum(lane_max < L <= wave_max for L in lengths)
            assert st["block_lists"] == sum(L > wave_max for L in lengths) >= 5
        else:
            assert st["lane_lists"] == len(lengths) and st["wave_lists"] == st["block_lists"] == 0
        assert st["decrements"] == sum(lengths)   # (the lists of the last pick are not walked: the row retires with it)
        # every holder of a shared hash lost it: after the hub only `second` is worth a pick
        assert [int(p["ref"]) for p in picks] == [hub, second] and [int(p["fresh"]) for p in picks] == [len(lengths), 3]
        assert n_cand.tolist() == [N_SEAM] and st["rounds"] == 2
    monkeypatch.delenv("RK_GATHER_SPLIT")


# ---- 6. many rounds, many candidates --------------------------------------------------------------------------------------------------------
def private_hash_collection(n, seed):
    """n references of 3 hashes each; the query holds ONE private hash of each"""
    pool = np.random.default_rng(seed).permutation(1 << 22)[: 3 * n].astype(np.uint32)
    refs = [np.sort(pool[3 * v: 3 * v + 3]) for v in range(n)]
    return refs, np.sort(pool[::3])


def test_many_rounds_one_private_hash_each(ctx):
    refs, query = private_hash_collection(600, 21)
    idx, qs = index_of(ctx, refs), queries_of(ctx, [query])
    (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, qs, refs, [query])
    assert picks["ref"].tolist() == list(range(600)) and set(picks["fresh"].tolist()) == {1} and picks["left"].tolist() == list(range(599, -1, -1))
    assert st["rounds"] == 600 and st["read_backs"] <= 2 + -(-600 // st["sync_every"]) and st["compactions"] >= 1
    (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, qs, refs, [query], max_picks=10)
    assert picks["ref"].tolist() == list(range(10)) and covered.tolist() == [10] and n_cand.tolist() == [600] and st["rounds"] == 10


def test_more_candidates_than_one_workgroup_has_threads(ctx):
    refs, query = private_hash_collection(3000, 22)
    refs[2500] = np.sort(np.concatenate([refs[2500], np.intersect1d(refs[7], query), np.intersect1d(refs[1999], query)]))   # one reference worth 3, far behind the first chunk
    idx, qs = index_of(ctx, refs), queries_of(ctx, [query])
    threads = constants(ctx)[2]
    assert 3000 > 4 * threads
    (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, qs, refs, [query], max_picks=5)
    assert picks["ref"].tolist() == [2500, 0, 1, 2, 3] and picks["fresh"].tolist() == [3, 1, 1, 1, 1] and n_cand.tolist() == [3000]
    (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, qs, refs, [query], min_new=2)
    assert picks["ref"].tolist() == [2500] and n_cand.tolist() == [1] and covered.tolist() == [3] and matched.tolist() == [3000]


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_rows_around_one_chunk_of_the_scan(ctx, delta):
    """k_query_scan (rk_query_dev.h, shared with rk_screen_rows) takes the rows in chunks of the workgroup's threads with a carry:
    threads - 1, threads and threads + 1 rows in one batch, so that its scans -- the candidates, their room capped at max_picks, the
    picks, and off[] over all rows -- end inside, at and one behind a chunk.  Row q holds a private hash of reference q % 8 and, when q
    is odd, one of the next reference: one or two candidates, of which max_picks = 1 keeps one"""
    threads = constants(ctx)[2]
    pool = np.random.default_rng(23).permutation(1 << 22)[:800].astype(np.uint32)
    refs = [np.sort(pool[100 * v: 100 * v + 100]) for v in range(8)]
    queries = [np.sort(pool[[100 * (q % 8) + q // 8] + ([100 * ((q + 1) % 8) + q // 8] if q % 2 else [])]) for q in range(threads + delta)]
    assert threads // 8 < 100
    (off, picks, matched, n_cand, covered), st = gathered(ctx, index_of(ctx, refs), queries_of(ctx, queries), refs, queries, max_picks=1)
    assert st["batches"] == 1 and off.tolist() == list(range(threads + delta + 1)) and n_cand.tolist() == [1 + q % 2 for q in range(threads + delta)]


# ---- 7. batches, shards, the host leg ---------------------------------------------------------------------------------------------------------
def test_batches_give_the_bytes_of_one_batch(ctx, monkeypatch):
    refs, queries, bits = clades(False)
    idx = index_of(ctx, refs, False, bits)
    qs = queries_of(ctx, queries)
    whole, st = gathered(ctx, idx, qs, refs, queries, want=wanted(False, 1, 0))
    assert st["batches"] == 1 and st["rows_per_batch"] == len(queries)
    monkeypatch.setenv("RK_GATHER_BATCH_BYTES", "1")   # less than a row: one row per batch
    single, st = gathered(ctx, idx, qs, refs, queries, want=wanted(False, 1, 0))
    assert st["batches"] == len(queries) and st["rows_per_batch"] == 1 and result_bytes(single) == result_bytes(whole)
    monkeypatch.setenv("RK_GATHER_BATCH_BYTES", str(64 << 10))
    some, st = gathered(ctx, idx, qs, refs, queries, want=wanted(False, 1, 0))
    per = st["rows_per_batch"]
    assert 2 <= per < len(queries) // 2 and result_bytes(some) == result_bytes(whole)
    n = len(queries) // per * per - 1 if len(queries) % per == 0 else len(queries)   # a last batch that is short
    short = queries[:n]
    want = wanted(False, 1, 0)[:n]
    part, st = gathered(ctx, idx, queries_of(ctx, short), refs, short, want=want)
    assert st["rows_per_batch"] == per and n % per != 0 and st["batches"] == n // per + 1
    monkeypatch.delenv("RK_GATHER_BATCH_BYTES")
    assert result_bytes(part) == result_bytes(gathered(ctx, idx, queries_of(ctx, short), refs, short, want=want)[0])


@pytest.mark.parametrize("block", [1, 3])
def test_row_shards_concatenate_to_the_whole(ctx, block):
    refs, queries, bits = clades(False)
    idx = index_of(ctx, refs, False, bits)
    qs = queries_of(ctx, queries)
    want = wanted(False, 2, 3)
    whole, _ = gathered(ctx, idx, qs, refs, queries, 2, 3, want=want)
    out = tuple(np.full(len(queries), 0xDEAD, dtype=np.uint32) for _ in range(3))
    parts = []
    for first in (0, 1):
        (off, picks, m, c, v), st = gathered(ctx, idx, qs, refs, queries, 2, 3, want=want, row_first=first, row_step=2, row_block=block)
        parts.append(picks)
        rows = ga.selected_rows(len(queries), first, 2, block)
        got = ctx.gather_rows(idx, qs, 2, 3, row_first=first, row_step=2, row_block=block, out=out)   # one set of arrays for both shards
        assert all(a is b for a, b in zip(got[2:5], out)) and len(rows) in (len(queries) // 2, len(queries) - len(queries) // 2)
    both = np.concatenate(parts)
    both = both[np.lexsort((both["rank"], both["query"]))]
    assert both.tobytes() == whole[1].tobytes() and all(np.array_equal(a, b) for a, b in zip(out, whole[2:]))


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("rows_per_batch", [1, 3])
def test_shards_with_a_partial_last_block_in_batches(ctx, monkeypatch, rows_per_batch, sliced):
    """23 rows in blocks of 4 dealt to 3 shards: block 5 (rows 20 .. 22) is partial and belongs to shard 2.  Batches of one row, and of
    three (a batch boundary inside every block), of rk_distq_counts(slot_base, n_slots) -- also over the sliced membership pass, which
    the later batches of a call reuse."""
    refs, queries, bits = clades(False)
    queries, want = queries[:23], wanted(False, 1, 0)[:23]
    idx = index_of(ctx, refs, False, bits)
    qs = queries_of(ctx, queries)
    row_bytes = 12 * len(refs) + 16 * max(len(q) for q in queries) + 64   # rk_gather.hip: counter row, candidates, items twice, state
    plain_name = ctx.dist_kernel_name(idx, qs, 0, 0, 20, 1.0)
    for first in range(3):
        shard = dict(row_first=first, row_step=3, row_block=4)
        one, st = gathered(ctx, idx, qs, refs, queries, want=want, **shard)
        assert st["batches"] == 1 and st["rows"] == (8, 8, 7)[first] == st["rows_per_batch"]
        monkeypatch.setenv("RK_GATHER_BATCH_BYTES", str(rows_per_batch * row_bytes + row_bytes // 2))
        if sliced:
            monkeypatch.setenv("RK_DISTQ_SLICED", "1")
            assert ctx.dist_kernel_name(idx, qs, 0, 0, 20, 1.0) != plain_name   # the pre-resolved look-up is what runs
        many, st = gathered(ctx, idx, qs, refs, queries, want=want, **shard)
        assert st["rows_per_batch"] == rows_per_batch and st["batches"] == -(-st["rows"] // rows_per_batch) >= 3
        assert result_bytes(many) == result_bytes(one) and len(many[1]) > 8
        monkeypatch.delenv("RK_GATHER_BATCH_BYTES")
        monkeypatch.delenv("RK_DISTQ_SLICED", raising=False)
    assert ga.selected_rows(23, 2, 3, 4)[-3:] == [20, 21, 22]


def test_host_leg_gives_the_same_bytes(ctx, monkeypatch):
    for wide in (False, True):
        refs, queries, bits = clades(wide)
        qs = queries_of(ctx, queries, wide)
        for make in (index_of, imported_index):
            idx = make(ctx, refs, wide, bits)
            for min_new, max_picks in ((1, 0), (2, 3)):
                device, st = gathered(ctx, idx, qs, refs, queries, min_new, max_picks, want=wanted(wide, min_new, max_picks))
                monkeypatch.setenv("RK_GATHER_DEVICE", "0")
                host, st2 = gathered(ctx, idx, qs, refs, queries, min_new, max_picks, path=2, want=wanted(wide, min_new, max_picks))
                shard, _ = gathered(ctx, idx, qs, refs, queries, min_new, max_picks, path=2, want=wanted(wide, min_new, max_picks), row_first=1, row_step=2, row_block=3)
                monkeypatch.delenv("RK_GATHER_DEVICE")
                assert result_bytes(host) == result_bytes(device)
                assert {k: st2[k] for k in ("picks", "candidates", "matched", "rows", "rounds")} == {k: st[k] for k in ("picks", "candidates", "matched", "rows", "rounds")}


def test_timed_span(ctx, monkeypatch):
    refs, queries, bits = clades(False)
    idx, qs = index_of(ctx, refs, False, bits), queries_of(ctx, queries)
    ctx.set_timing(True)
    gathered(ctx, idx, qs, refs, queries, want=wanted(False, 1, 0))
    assert ctx.last_ms(capi.MS_GATHER) > 0.0
    monkeypatch.setenv("RK_GATHER_DEVICE", "0")
    gathered(ctx, idx, qs, refs, queries, path=2, want=wanted(False, 1, 0))
    monkeypatch.delenv("RK_GATHER_DEVICE")
    assert ctx.last_ms(capi.MS_GATHER) == 0.0
    ctx.set_timing(False)


# ---- 8. the empty cases ---------------------------------------------------------------------------------------------------------------------
def test_empty_cases(ctx):
    refs, queries, bits = clades(False)
    idx = index_of(ctx, refs, False, bits)
    empty, foreign = queries[-2], queries[-1]
    assert len(empty) == 0 and len(foreign) > 10
    for qset in ([empty], [foreign], [empty, foreign, refs[5], empty]):
        (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, queries_of(ctx, qset), refs, qset)
        assert st["batches"] == 1 and len(picks) == (1 if len(qset) == 4 else 0)
    # Q = 0: nothing runs
    none_q = ctx.sketches_from_host(np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64))
    (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, none_q, refs, [], path=0)
    assert off.tolist() == [0] and len(picks) == len(matched) == 0 and st["path"] == 0
    # an index without genomes: every row empty
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 24)
    qset = [refs[0], empty]
    (off, picks, matched, n_cand, covered), st = gathered(ctx, none, queries_of(ctx, qset), [], qset, path=0)
    assert off.tolist() == [0, 0, 0] and len(picks) == 0 and matched.tolist() == [0, 0] and st["rows"] == 2
    # a row shard that selects nothing
    (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, queries_of(ctx, qset), refs, qset, path=0, row_first=5, row_step=7, row_block=1)
    assert off.tolist() == [0, 0, 0] and st["rows"] == 0


# ---- 9. the round trip from rk_group_sketches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_a_pan_sketch_is_covered_entirely_by_its_own_collection(ctx, wide):
    refs, _, bits = clades(wide)
    idx = index_of(ctx, refs, wide, bits)
    labels = [(v * 7919) % len(refs) // 125 * 125 for v in range(len(refs))]   # 8 groups of 125 genomes
    sk, gl, gs, gst = ctx.group_sketches(idx, labels, "pan")
    assert sk.count == len(gl) == 8
    h, off = sk.download()
    pans = ga.parts_of(h, off)
    (off, picks, matched, n_cand, covered), st = gathered(ctx, idx, sk, refs, pans)
    sizes = [len(p) for p in pans]
    assert matched.tolist() == covered.tolist() == sizes and min(sizes) > 1000
    for q in range(8):   # every hash of a pan sketch is some member's: nothing is left
        mine = picks[picks["query"] == q]
        assert len(mine) >= 2 and mine["left"][-1] == 0 and mine["fresh"].sum() == sizes[q]


# ---- 10. what is refused ----------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, idx, qs, opts=(1, 0, 0, 0, 0), skip=None):
    L = capi.lib()
    L.rk_gather_rows.argtypes = ROWS_ARGTYPES
    q = qs.count if qs is not None else 2
    off = np.full(q + 1, 0x77, dtype=np.uint64)
    outs = [np.full(q, 0x55, dtype=np.uint32) for _ in range(3)]
    picks, n = C.c_void_p(0x1234), C.c_uint64(0xABAB)
    o = capi.GatherOpts(*opts) if opts is not None else None
    args = [ctx._h, idx._h if idx is not None else None, qs._h if qs is not None else None, C.byref(o) if o is not None else None, off.ctypes.data,
            C.byref(picks), C.byref(n), outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, C.byref(capi.GatherStats())]
    if skip is not None:
        args[skip] = None
    rc = L.rk_gather_rows(*args)
    return rc, picks.value == 0x1234 and n.value == 0xABAB and bool((off == 0x77).all()) and all(bool((a == 0x55).all()) for a in outs)


def test_arguments_that_are_refused(ctx):
    refs, queries, bits = clades(False)
    idx, qs = index_of(ctx, refs, False, bits), queries_of(ctx, queries)
    last = lambda: capi.lib().rk_last_error(ctx._h)   # noqa: E731
    assert raw_call(ctx, idx, qs, (0, 0, 0, 0, 0)) == (RK_ERR_ARG, True) and b"min_new" in last()
    assert raw_call(ctx, idx, qs, None) == (RK_ERR_ARG, True)
    for skip in (1, 2, 4, 5, 6, 7, 8, 9):   # idx, queries, off_out, picks_out, n_picks, matched_out, n_cand_out, covered_out
        assert raw_call(ctx, idx, qs, skip=skip) == (RK_ERR_ARG, True), skip
    wrefs, wqueries, wbits = clades(True)
    assert raw_call(ctx, idx, queries_of(ctx, wqueries, True)) == (RK_ERR_ARG, True) and b"widths" in last()
    assert raw_call(ctx, index_of(ctx, wrefs, True, wbits), qs) == (RK_ERR_ARG, True) and b"widths" in last()
    # sketches that repeat a hash: queries, then references
    twice = ctx.sketches_from_host(np.array([5, 5, 9], dtype=np.uint32), np.array([0, 3], dtype=np.uint64))
    assert raw_call(ctx, idx, twice) == (RK_ERR_UNSUPPORTED, True) and b"sets" in last()
    assert raw_call(ctx, ctx.index_build(twice, 24), qs) == (RK_ERR_UNSUPPORTED, True) and b"sets" in last()
    with pytest.raises(capi.RkError) as e:
        ctx.gather_rows(idx, qs, min_new=0)
    assert e.value.code == RK_ERR_ARG
    with pytest.raises(ValueError):
        ctx.gather_rows(idx, qs, out=(np.zeros(3, dtype=np.uint32),) * 3)
    assert raw_call(ctx, idx, qs)[0] == 0   # and the good call runs (its picks are the library's: leaked here, a few KB)


def test_indexes_without_all_posting_lists_are_refused(ctx):
    import torch
    S = 2
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    sk = ctx.sketches_from_host(h, off)
    qs = queries_of(ctx, ga.parts_of(h, off)[:3])
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    assert raw_call(ctx, parts[0], qs) == (RK_ERR_ARG, True)   # one hash range of a sharded build
    assert b"posting lists" in capi.lib().rk_last_error(ctx._h)
    sent = [p.shard_records(S) for p in parts]
    bufs = []
    for p, cnt in zip(parts, sent):
        b = torch.empty(max(1, sum(cnt) * 12), dtype=torch.uint8, device="cuda")
        p.shard_pack(b.data_ptr())
        bufs.append(b)
    torch.cuda.synchronize()
    recv = torch.cat([bufs[r][: 12 * sent[r][0]] for r in range(S)] + [torch.empty(1, dtype=torch.uint8, device="cuda")])
    torch.cuda.synchronize()
    j = ctx.index_join_shard(parts[0], recv.data_ptr(), sum(sent[r][0] for r in range(S)))
    assert raw_call(ctx, j, qs) == (RK_ERR_ARG, True)   # the join-only index: tile records of its rows, no lists
    assert b"posting lists" in capi.lib().rk_last_error(ctx._h)
    del j, parts, sk


# ---- 11. the tool -----------------------------------------------------------------------------------------------------------------------------
def run_tool(cwd, args):
    return subprocess.run([TOOL, "gather"] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_tool_gather_subcommand(ctx, tmp_path):
    rnames, refs, qnames, queries, triples = golden_pair("32")
    shutil.copy(os.path.join(GOLDEN, "dist", "ref.sketch"), tmp_path / "ref.sketch")
    shutil.copy(os.path.join(GOLDEN, "dist", "qry.sketch"), tmp_path / "qry.sketch")
    for extra, min_new, max_picks in (([], 1, 0), (["--min-new", "5", "--max-picks", "2"], 5, 2)):
        p = run_tool(tmp_path, ["-r", "ref.sketch", "-q", "qry.sketch", "-o", "out.txt", "--summary", "sum.txt"] + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        want = ga.fast(refs, queries, min_new, max_picks)
        off, picks, matched, n_cand, covered = ga.as_arrays(want, refs, queries)
        assert len(picks) >= 5
        lines = (tmp_path / "out.txt").read_text().splitlines()
        assert lines == ["%s\t%s\t%d\t%d|%d|%d\t%d\t%s\t%s" % (qnames[q], rnames[r], rank, common, sr, sq, fresh, "%f" % (fresh / sq), "%f" % (common / sr))
                         for q, r, rank, common, fresh, left, sr, sq in picks]
        for line in lines:   # the triple is the real reference's
            f = line.split("\t")
            assert tuple(int(x) for x in f[3].split("|")) == triples[(f[0], f[1])]
        assert (tmp_path / "sum.txt").read_text().splitlines() == ["%s\t%d\t%d\t%d\t%d\t%d" % (qnames[q], len(queries[q]), matched[q], covered[q], n_cand[q], off[q + 1] - off[q])
                                                                   for q in range(len(queries))]
    # what dies, with a message, before a file is written
    for args, text in ((["-r", "ref.sketch", "-o", "x.txt"], b"needs -r and -q"), (["-q", "qry.sketch", "-o", "x.txt"], b"needs -r and -q"),
                       (["-r", "ref.sketch", "-q", "qry.sketch", "-o", "x.txt", "--gpus", "2"], b"one GPU"),
                       (["-r", "ref.sketch", "-q", "qry.sketch", "-o", "x.txt", "--min-new", "0"], b"--min-new must be >= 1")):
        p = run_tool(tmp_path, args)
        assert p.returncode != 0 and text in p.stderr and not (tmp_path / "x.txt").exists(), args
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"gather -r" in p.stderr and b" sub gather convert " in p.stderr
