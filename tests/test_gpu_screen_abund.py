"""rk_screen_abund_rows on the device against tests/_screen_abund_ref.py: the golden pairs and random clades with seeded counts under both
hash widths, built and imported; one record per segment length at every bound of the select classes with won 0, 1, common - 1 and common
(read from the call's stats which class ran); the rounds of the radix select at their byte edges; the three walks of the fill at their
seams with a distinct count per hash; one cursor that takes every add; tiles and sketch boundaries; batches, value sub-ranges and row
shards; the host leg; the cross-checks inside the project; the refusals and the empty cases; `rabbit_kssd screen --abund`.  Every call is also compared byte for byte
with rk_screen_rows on the same sketches.  Every comparison is exact."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _screen_abund_ref as ar
import _screen_ref as sr
from _selfjoin_cases import TOOL, csr, device_index
from conftest import GOLDEN
from rabbitkssd_amd import capi
from _screen_cases import clades, golden_pair, imported_index, index_of
from test_gpu_screen import FIRST_CHAMPION, N_SEAM, seam_collection

pytestmark = pytest.mark.gpu
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6
TOP = 2 ** 32 - 1


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def counted(ctx, queries, wide=False):
    """counted sketches from dicts hash -> count"""
    hs = [np.array(sorted(m), dtype=np.uint64 if wide else np.uint32) for m in queries]
    cs = [np.array([m[int(h)] for h in p], dtype=np.uint32) for m, p in zip(queries, hs)]
    h, off = csr(hs, np.uint64 if wide else np.uint32)
    c = np.concatenate(cs).astype(np.uint32) if cs else np.zeros(0, dtype=np.uint32)
    return ctx.sketches_from_host_counts(h, c, off, wide=wide)


def classes(commons, st):
    return (sum(c <= st["rank_max"] for c in commons), sum(st["rank_max"] < c <= st["wave_sel_max"] for c in commons), sum(c > st["wave_sel_max"] for c in commons))


def screened(ctx, idx, qs, refs, queries, min_common=1, min_won=0, path=1, want=None, **rows):
    """the call, with what every result must satisfy: the bytes of rk_screen_rows, and the reference exactly; returns (arrays, stats)"""
    got = ctx.screen_abund_rows(idx, qs, min_common, min_won, **rows)
    off, recs, abund, matched, n_cand, claimed, occ, st = got
    plain = ctx.screen_rows(idx, qs, min_common, min_won, **rows)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((off, recs, matched, n_cand, claimed), plain[:5]))
    sel = sr.selected_rows(len(queries), rows.get("row_first", 0), rows.get("row_step", 1), rows.get("row_block", 0))
    result = want if want is not None else ar.fast(refs, queries, min_common, min_won)
    w_off, w_recs, w_abund, w_matched, w_cand, w_claimed, w_occ = ar.as_arrays(result, refs, queries, sel)
    assert st["path"] == path and st["rows"] == len(sel) and plain[5]["path"] == path
    assert off.tolist() == w_off and sr.rec_tuples(recs) == w_recs
    assert matched.tolist() == w_matched and n_cand.tolist() == w_cand and claimed.tolist() == w_claimed
    assert ar.abund_tuples(abund) == w_abund
    assert occ.tolist() == w_occ
    assert (st["rank_max"], st["wave_sel_max"], st["chunk"]) == (64, st["wave_sel_max"], st["threads"]) and st["wave_sel_max"] > 64
    if path == 0:
        assert st["values"] == st["value_passes"] == st["launches"] == 0
        return got[:7], st
    same = ("records", "candidates", "matched", "claimed", "postings_walked", "lane_lists", "wave_lists", "block_lists", "rows", "batches", "read_backs")
    assert {k: st[k] for k in same} == {k: plain[5][k] for k in same}   # one read-back per batch, as the plain screen
    commons = [t[2] for t in w_recs]
    assert st["values"] == sum(commons) and (st["rank_segs"], st["wave_segs"], st["block_segs"]) == classes(commons, st)
    if path == 1:
        assert st["value_passes"] >= st["batches"] >= 1 and st["value_bytes"] > 0
    else:
        assert st["value_passes"] == 0 and st["launches"] == 0
    return got[:7], st


def result_bytes(arrays):
    return b"".join(a.tobytes() for a in arrays)


def seeded_counts(parts, seed):
    return ar.with_counts(parts, np.random.default_rng(seed))


# ---- 1. golden pairs and clades -------------------------------------------------------------------------------------------------------
OPTIONS = [(1, 0), (3, 0), (1, 2), (3, 2)]


@pytest.mark.parametrize("tag,how", [("32", "built"), ("32", "imported"), ("64", "built"), ("64", "imported")])
def test_golden_pairs_with_seeded_counts(ctx, tag, how):
    rnames, refs, qnames, queries, triples = golden_pair(tag)
    wide, bits = (True, 36) if tag == "64" else (False, 24)
    idx = (index_of if how == "built" else imported_index)(ctx, refs, wide, bits)
    qd = seeded_counts(queries, 5)
    qs = counted(ctx, qd, wide)
    for min_common, min_won in OPTIONS:
        (off, recs, abund, matched, n_cand, claimed, occ), st = screened(ctx, idx, qs, refs, qd, min_common, min_won)
        assert len(recs) >= 1 and st["batches"] == 1
        for p in recs:   # the real reference's intersection count of that pair
            assert int(p["common"]) == triples[(qnames[p["query"]], rnames[p["ref"]])][0]


_wanted = {}


def clade_case(wide):
    """clades(wide) with seeded counts and the reference's answers, computed once and shared"""
    if wide not in _wanted:
        refs, queries, bits = clades(wide)
        qd = seeded_counts(queries, 23 + wide)
        _wanted[wide] = (refs, qd, bits, {o: ar.fast(refs, qd, *o) for o in OPTIONS + [(2, 1)]})
    return _wanted[wide]


@pytest.mark.parametrize("wide", [False, True])
def test_random_clades_under_every_option(ctx, wide):
    refs, qd, bits, want = clade_case(wide)
    idx = index_of(ctx, refs, wide, bits)
    assert not np.array_equal(idx.order, np.arange(len(refs)))   # internal order != caller order
    qs = counted(ctx, qd, wide)
    for o in OPTIONS:
        arrays, st = screened(ctx, idx, qs, refs, qd, *o, want=want[o])
        assert st["batches"] == 1
    ar.facts(refs, qd, want[(1, 0)])
    a, _ = screened(ctx, idx, qs, refs, qd, want=want[(1, 0)])
    b, _ = screened(ctx, imported_index(ctx, refs, wide, bits), qs, refs, qd, want=want[(1, 0)])
    assert result_bytes(a) == result_bytes(b)   # built and imported: the same bytes


# ---- 2. segment lengths and the radix rounds ---------------------------------------------------------------------------------------------
class Rows:
    """One query row and two references per case, every case with hashes of its own: A holds `length` hashes, all in the query; B holds
    length - won of them and won + 1 hashes of its own, all in the query too -- both containments are 1, B is the larger: it takes what
    it shares, A keeps exactly `won`.  counts[i] is the count of A's hash i; B's own hashes count 1."""

    def __init__(self):
        self.refs, self.queries, self.expect, self.next = [], [], [], 1000

    def add(self, length, won, counts):
        assert 0 <= won <= length == len(counts)
        mine = list(range(self.next, self.next + length))
        own = list(range(self.next + length, self.next + length + won + 1))
        self.next += 2 * length + 10
        self.refs += [mine, mine[won:] + own]
        q = dict(zip(mine, (int(c) for c in counts)))
        q.update({h: 1 for h in own})
        self.queries.append(q)
        self.expect.append((length, won))

    def run(self, ctx, **kw):
        idx = index_of(ctx, [np.array(r, dtype=np.uint32) for r in self.refs])
        want = ar.fast(self.refs, self.queries)
        for q, (length, won) in enumerate(self.expect):   # the construction does what it says
            assert want[q][0] == [(q, 2 * q, length, won), (q, 2 * q + 1, length + 1, length + 1)]
        return screened(ctx, idx, counted(ctx, self.queries), self.refs, self.queries, want=want, **kw)


def constants(ctx):
    one = [np.array([1], dtype=np.uint32)]
    st = ctx.screen_abund_rows(index_of(ctx, one), counted(ctx, [{1: 1}]))[7]
    return st["rank_max"], st["wave_sel_max"], st["chunk"]


def test_one_record_per_segment_length_at_every_bound_of_the_select_classes(ctx):
    rank_max, wave_sel_max, chunk = constants(ctx)
    assert rank_max == 64 and wave_sel_max % chunk == 0
    lengths = [1, 2, 3] + [b + d for b in (rank_max, wave_sel_max) for d in (-1, 0, 1)] + [wave_sel_max + 4 * chunk + 1]
    rng = np.random.default_rng(41)
    rows = Rows()
    for n in lengths:
        for won in sorted({0, 1, n - 1, n}):
            rows.add(n, won, rng.integers(1, 1 << 20, size=n))   # (nearly) distinct values: a misplaced one moves a median or a sum
    (off, recs, abund, matched, n_cand, claimed, occ), st = rows.run(ctx)
    commons = [n + k for n, won in rows.expect for k in (0, 1)]   # A and B of every case
    assert (st["rank_segs"], st["wave_segs"], st["block_segs"]) == classes(commons, st)
    assert st["rank_segs"] >= 20 and st["wave_segs"] >= 20 and st["block_segs"] >= 12   # every class ran, on every kind of won
    # lower medians: two values, all equal, two distinct values half and half -- in every class
    rows = Rows()
    for n in (2, 4, rank_max, rank_max + 2, wave_sel_max, wave_sel_max + 2):
        half = [7] * (n // 2) + [9] * (n // 2)
        for counts in (half, half[::-1], [5] * n, [9, 7] * (n // 2)):
            for won in (0, n // 2, n):
                rows.add(n, won, counts)
    (off, recs, abund, matched, n_cand, claimed, occ), st = rows.run(ctx)
    for q, (n, won) in enumerate(rows.expect):
        a = abund[int(off[q])]
        assert int(a["med_common"]) in (5, 7) and int(a["med_won"]) in (0, 5, 7, 9)
    assert abund["med_common"][0] == 7 and abund["med_won"][0] == 0   # (7, 9), nothing claimed


def test_the_rounds_of_the_radix_select_at_their_byte_edges(ctx):
    rank_max, wave_sel_max, chunk = constants(ctx)
    rng = np.random.default_rng(43)
    rows = Rows()
    for n in (rank_max - 3, 3 * rank_max + 1, wave_sel_max + chunk + 3):   # ranked in registers; a wave's radix select; the workgroup's
        edges = [255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, TOP, TOP - 1, 1]
        patterns = [
            (rng.integers(1, 256, size=n).astype(np.uint64) << 24) | 0x00ABCDEF,   # only the top byte differs
            0x12345600 | rng.integers(0, 256, size=n).astype(np.uint64),           # only the lowest byte
            0x12005678 | (rng.integers(0, 256, size=n).astype(np.uint64) << 16),   # only the second byte
            rng.choice(edges, size=n),                                             # both sides of every round's boundary, and the largest count
            np.array([TOP] * 3 + [1] * (n - 3)),                                   # three counts of 2^32 - 1: a sum beyond 2^32
            np.full(n, TOP),
        ]
        for counts in patterns:
            for won in (0, n // 3, n):
                rows.add(n, won, rng.permutation(counts))
    (off, recs, abund, matched, n_cand, claimed, occ), st = rows.run(ctx)
    assert st["rank_segs"] and st["wave_segs"] and st["block_segs"] and int(abund["occ_common"].max()) > 2 ** 32 * 1000
    assert int(abund["med_common"].max()) == TOP


# ---- 3. the walks of the fill -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["imported", "built"])
def test_every_walk_of_the_fill_at_its_seams(ctx, how):
    one = [np.array([1], dtype=np.uint32)]
    st = ctx.screen_rows(index_of(ctx, one), counted(ctx, [{1: 1}]))[5]
    lane_max, wave_max, threads = st["lane_max"], st["wave_max"], st["threads"]
    refs, query, plan, lengths, (only_last, nobody, last_holder) = seam_collection(lane_max, wave_max, threads)
    idx = (imported_index if how == "imported" else index_of)(ctx, [r for r in refs], False, 24)
    qd = [{int(h): 1000 + 7 * i for i, h in enumerate(query)}]   # a distinct count per hash: a misplaced value changes a sum or a median
    qs = counted(ctx, qd)
    (off, recs, abund, matched, n_cand, claimed, occ), st = screened(ctx, idx, qs, refs, qd)
    assert st["lane_lists"] and st["wave_lists"] and st["block_lists"] >= 21 and len(recs) > 2000
    by_ref = {int(r["ref"]): (int(r["won"]), int(a["occ_won"]), int(a["occ_common"])) for r, a in zip(recs, abund)}
    for s, n, where, champion in plan:   # every champion claims its one hash, whichever walk found it and wherever it sat in the list
        assert by_ref[champion] == (1, qd[0][int(s)], qd[0][int(s)])
    # min_common = 2: `only_last` goes to the last posting of its list, the only holder with a record; `nobody`'s list has none
    (off, recs, abund, matched, n_cand, claimed, occ), st = screened(ctx, idx, qs, refs, qd, 2)
    by_ref = {int(r["ref"]): int(a["occ_won"]) for r, a in zip(recs, abund)}
    assert by_ref[last_holder] > qd[0][int(only_last)] and all(v not in by_ref for v in range(FIRST_CHAMPION + 94, FIRST_CHAMPION + 98))
    assert occ[0][2] < occ[0][1] and N_SEAM == len(refs)


def test_one_front_cursor_takes_every_add_and_one_record_only_its_back(ctx):
    rng = np.random.default_rng(8)
    pool = rng.permutation(1 << 23)[:4000].astype(np.uint32)
    core = pool[:100]
    strains = [np.sort(np.concatenate([core, pool[100 + 10 * v: 110 + 10 * v]])) for v in range(300)]
    hub = 137
    strains[hub] = np.sort(pool[:100 + 10 * 300])   # holds what every strain holds: it wins everything
    qd = [{int(h): int(c) for h, c in zip(strains[hub], rng.integers(1, 1 << 16, size=len(strains[hub])))}]
    idx, qs = index_of(ctx, strains), counted(ctx, qd)
    (off, recs, abund, matched, n_cand, claimed, occ), st = screened(ctx, idx, qs, strains, qd)
    assert len(recs) == 300 and int(recs[hub]["won"]) == 3100 and st["block_segs"] == 1 and st["wave_segs"] == 299
    assert int(abund[hub]["occ_won"]) == int(abund[hub]["occ_common"]) == sum(qd[0].values()) == int(occ[0][2])
    assert all(int(a["occ_won"]) == 0 and int(a["med_won"]) == 0 and int(a["med_common"]) > 0 for v, a in enumerate(abund) if v != hub)


# ---- 4. tiles and rows -----------------------------------------------------------------------------------------------------------------
def test_sketch_boundaries_around_tiles_and_lane_seams(ctx):
    tile = ctx.screen_rows(index_of(ctx, [np.array([1], dtype=np.uint32)]), counted(ctx, [{1: 1}]))[5]["tile_hashes"]
    rng = np.random.default_rng(15)
    pool = rng.permutation(1 << 23).astype(np.uint32)
    universe, foreign = pool[:3000], pool[3000:8000]
    refs = [np.sort(rng.choice(universe, size=int(rng.integers(30, 90)), replace=False)) for _ in range(40)]
    indexed = np.unique(np.concatenate(refs))
    sizes = [63, 1, 1, 0, 0, 0, tile - 66, 1, 1, 1, 0, 0, 0, tile - 2, 1, 1, 2 * tile, 5, 0]
    ends = np.cumsum(sizes).tolist()
    assert {63, 64, 65, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1}.issubset(ends) and len(indexed) >= tile
    queries = []
    for k, n in enumerate(sizes):
        src = indexed if k % 3 == 0 and n <= len(indexed) else foreign if k % 3 == 1 else np.concatenate([indexed[:1500], foreign[:1500]])
        queries.append(np.sort(rng.choice(src, size=n, replace=False)).astype(np.uint32))
    idx = index_of(ctx, refs)
    qd = seeded_counts(queries, 3)
    screened(ctx, idx, counted(ctx, qd), refs, qd)
    for shift in (1, 62, tile - 63):   # the same sketches behind a first one that moves every boundary
        moved = seeded_counts([np.sort(rng.choice(indexed, size=shift, replace=False)).astype(np.uint32)], shift) + qd
        screened(ctx, idx, counted(ctx, moved), refs, moved)
    for qset in ([qd[3]], [qd[3]] * 5, [qd[13]], [qd[3], qd[16], qd[3]]):   # empty sketches only; no match at all
        screened(ctx, idx, counted(ctx, qset), refs, qset)


# ---- 5. batches, value sub-ranges, shards, the host leg -----------------------------------------------------------------------------------
def test_batches_and_value_sub_ranges_give_the_bytes_of_one(ctx, monkeypatch):
    refs, qd, bits, want = clade_case(False)
    qd, w = qd[:7], want[(1, 0)][:7]
    idx, qs = index_of(ctx, refs, False, bits), counted(ctx, qd)
    whole, st = screened(ctx, idx, qs, refs, qd, want=w)
    assert st["batches"] == 1 and st["rows_per_batch"] == 7 and st["value_passes"] == 1
    row_bytes = 8 * len(refs) + 16
    monkeypatch.setenv("RK_SCREEN_BATCH_BYTES", str(3 * row_bytes + row_bytes // 2))
    some, st = screened(ctx, idx, qs, refs, qd, want=w)
    assert st["rows_per_batch"] == 3 and st["batches"] == 3 == st["value_passes"] and result_bytes(some) == result_bytes(whole)
    monkeypatch.delenv("RK_SCREEN_BATCH_BYTES")
    per_row = [sum(t[2] for t in x[0]) for x in w]   # the values of every row
    assert min(per_row) > 0
    # a budget of the two largest rows: several sub-ranges of the one batch; the reference says how many (rows are taken while they fit)
    budget = 4 * sum(sorted(per_row)[-2:])
    passes, run = 1, 0
    for v in per_row:
        if run and (run + v) * 4 > budget:
            passes, run = passes + 1, 0
        run += v
    monkeypatch.setenv("RK_SCREEN_VALUE_BYTES", str(budget))
    some, st = screened(ctx, idx, qs, refs, qd, want=w)
    assert st["batches"] == 1 and 1 < st["value_passes"] == passes < 7 and st["value_bytes"] == budget and result_bytes(some) == result_bytes(whole)
    monkeypatch.setenv("RK_SCREEN_VALUE_BYTES", "4")   # less than any row: one row per sub-range
    single, st = screened(ctx, idx, qs, refs, qd, want=w)
    assert st["batches"] == 1 and st["value_passes"] == 7 and result_bytes(single) == result_bytes(whole)
    monkeypatch.setenv("RK_SCREEN_BATCH_BYTES", str(3 * row_bytes))
    both, st = screened(ctx, idx, qs, refs, qd, 2, 1, want=want[(2, 1)][:7])
    assert st["batches"] == 3 and st["value_passes"] == 7
    monkeypatch.delenv("RK_SCREEN_BATCH_BYTES")
    monkeypatch.delenv("RK_SCREEN_VALUE_BYTES")


@pytest.mark.parametrize("block", [1, 3])
def test_row_shards_concatenate_to_the_whole(ctx, block):
    refs, qd, bits, want = clade_case(False)
    idx, qs = index_of(ctx, refs, False, bits), counted(ctx, qd)
    whole, _ = screened(ctx, idx, qs, refs, qd, 2, 1, want=want[(2, 1)])
    out = tuple(np.full(len(qd), 0xDEAD, dtype=np.uint32) for _ in range(3)) + (np.full((len(qd), 3), 0xDEAD, dtype=np.uint64),)
    recs, abund = [], []
    for first in (0, 1, 2):
        (off, r, a, m, c, v, o), st = screened(ctx, idx, qs, refs, qd, 2, 1, want=want[(2, 1)], row_first=first, row_step=3, row_block=block)
        recs.append(r)
        abund.append(a)
        rows = sr.selected_rows(len(qd), first, 3, block)
        before = [x.copy() for x in out]
        got = ctx.screen_abund_rows(idx, qs, 2, 1, row_first=first, row_step=3, row_block=block, out=out)   # one set of arrays for the shards
        assert all(x is y for x, y in zip(got[3:7], out))
        for x, y in zip(out, before):   # unselected entries are untouched
            assert all(np.array_equal(x[q], y[q]) for q in range(len(qd)) if q not in rows)
    recs, abund = np.concatenate(recs), np.concatenate(abund)
    order = np.lexsort((recs["ref"], recs["query"]))
    assert recs[order].tobytes() == whole[1].tobytes() and abund[order].tobytes() == whole[2].tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(out, whole[3:]))


def test_host_leg_gives_the_same_bytes(ctx, monkeypatch):
    for wide in (False, True):
        refs, qd, bits, want = clade_case(wide)
        qs = counted(ctx, qd, wide)
        for make in (index_of, imported_index):
            idx = make(ctx, refs, wide, bits)
            for o in ((1, 0), (3, 2)):
                device, st = screened(ctx, idx, qs, refs, qd, *o, want=want[o])
                monkeypatch.setenv("RK_SCREEN_DEVICE", "0")
                host, st2 = screened(ctx, idx, qs, refs, qd, *o, path=2, want=want[o])
                screened(ctx, idx, qs, refs, qd, *o, path=2, want=want[o], row_first=1, row_step=2, row_block=3)
                monkeypatch.delenv("RK_SCREEN_DEVICE")
                assert result_bytes(host) == result_bytes(device)
                same = ("records", "values", "rank_segs", "wave_segs", "block_segs", "matched", "claimed", "rows")
                assert {k: st2[k] for k in same} == {k: st[k] for k in same}


def test_timed_span(ctx, monkeypatch):
    refs, qd, bits, want = clade_case(False)
    idx, qs = index_of(ctx, refs, False, bits), counted(ctx, qd)
    ctx.set_timing(True)
    ctx.screen_abund_rows(idx, qs)
    assert ctx.last_ms(capi.MS_SCREEN_ABUND) > 0.0
    monkeypatch.setenv("RK_SCREEN_DEVICE", "0")
    ctx.screen_abund_rows(idx, qs)
    monkeypatch.delenv("RK_SCREEN_DEVICE")
    assert ctx.last_ms(capi.MS_SCREEN_ABUND) == 0.0
    ctx.set_timing(False)


# ---- 6. cross-checks inside the project ---------------------------------------------------------------------------------------------------
def test_with_all_counts_one_the_sums_are_the_cardinalities(ctx):
    refs, queries, bits = clades(False)
    ones = [{int(h): 1 for h in q} for q in queries]
    idx, qs = index_of(ctx, refs, False, bits), counted(ctx, ones)
    off, recs, abund, matched, n_cand, claimed, occ, st = ctx.screen_abund_rows(idx, qs, 2, 0)
    assert len(recs) > 100 and np.array_equal(abund["occ_common"], recs["common"]) and np.array_equal(abund["occ_won"], recs["won"])
    assert (abund["med_common"] == 1).all() and np.array_equal(abund["med_won"], (recs["won"] > 0).astype(np.uint32))
    assert occ[:, 0].tolist() == [len(q) for q in queries] and np.array_equal(occ[:, 1], matched) and np.array_equal(occ[:, 2], claimed)


def test_the_sum_of_the_whole_sketch_is_the_sum_of_its_downloaded_counts(ctx):
    refs, qd, bits, want = clade_case(True)
    idx, qs = index_of(ctx, refs, True, bits), counted(ctx, qd, True)
    counts, off = qs.download_counts(), qs.download()[1]
    occ = ctx.screen_abund_rows(idx, qs)[6]
    assert occ[:, 0].tolist() == [int(counts[int(off[q]):int(off[q + 1])].sum(dtype=np.uint64)) for q in range(len(qd))] and occ[:, 0].max() > 1000


# ---- 7. the empty cases and what is refused -------------------------------------------------------------------------------------------------
def test_empty_cases(ctx):
    refs, qd, bits, want = clade_case(False)
    idx = index_of(ctx, refs, False, bits)
    none_q = ctx.sketches_from_host_counts(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64))
    (off, recs, abund, matched, n_cand, claimed, occ), st = screened(ctx, idx, none_q, refs, [], path=0)
    assert off.tolist() == [0] and len(recs) == len(abund) == len(matched) == 0 and occ.shape == (0, 3)
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 24)   # an index without genomes: every row empty
    qset = [qd[0], qd[-1]]
    (off, recs, abund, matched, n_cand, claimed, occ), st = screened(ctx, none, counted(ctx, qset), [], qset, path=0)
    assert off.tolist() == [0, 0, 0] and len(abund) == 0 and occ.tolist() == [[sum(m.values()), 0, 0] for m in qset] and st["rows"] == 2
    (off, recs, abund, matched, n_cand, claimed, occ), st = screened(ctx, idx, counted(ctx, qset), refs, qset, path=0, row_first=5, row_step=7, row_block=1)
    assert off.tolist() == [0, 0, 0] and st["rows"] == 0 and occ.tolist() == [[0, 0, 0]] * 2
    # queries that match nothing, and a min_won nobody reaches: no record, the sums stay
    foreign = [{(1 << 24) + k: k + 1 for k in range(70)}]   # (beyond the 24 bits of the index)
    (off, recs, abund, matched, n_cand, claimed, occ), st = screened(ctx, idx, counted(ctx, foreign), refs, foreign)
    assert len(recs) == 0 and occ.tolist() == [[sum(range(1, 71)), 0, 0]]
    (off, recs, abund, matched, n_cand, claimed, occ), st = screened(ctx, idx, counted(ctx, qd[:3]), refs, qd[:3], 1, 10 ** 6)
    assert len(recs) == len(abund) == 0 and st["values"] == 0 and (occ[:, 2] > 0).all()


ROWS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.ScreenOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.ScreenAbundStats)]


def raw_call(ctx, idx, qs, opts=(1, 0, 0, 0, 0), skip=None):
    L = capi.lib()
    L.rk_screen_abund_rows.argtypes = ROWS_ARGTYPES
    q = qs.count if qs is not None else 2
    off = np.full(q + 1, 0x77, dtype=np.uint64)
    outs = [np.full(q, 0x55, dtype=np.uint32) for _ in range(3)]
    occ = np.full(3 * q, 0x33, dtype=np.uint64)
    recs, abund, n = C.c_void_p(0x1234), C.c_void_p(0x4321), C.c_uint64(0xABAB)
    o = capi.ScreenOpts(*opts) if opts is not None else None
    args = [ctx._h, idx._h if idx is not None else None, qs._h if qs is not None else None, C.byref(o) if o is not None else None, off.ctypes.data,
            C.byref(recs), C.byref(abund), C.byref(n), outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, occ.ctypes.data,
            C.byref(capi.ScreenAbundStats())]
    if skip is not None:
        args[skip] = None
    rc = L.rk_screen_abund_rows(*args)
    untouched = (recs.value == 0x1234 and abund.value == 0x4321 and n.value == 0xABAB and bool((off == 0x77).all()) and all(bool((a == 0x55).all()) for a in outs)
                 and bool((occ == 0x33).all()))
    return rc, untouched


def test_arguments_that_are_refused(ctx):
    refs, qd, bits, want = clade_case(False)
    idx, qs = index_of(ctx, refs, False, bits), counted(ctx, qd)
    last = lambda: capi.lib().rk_last_error(ctx._h)   # noqa: E731
    plain = ctx.sketches_from_host(*csr([np.array(sorted(m), dtype=np.uint32) for m in qd]))
    assert raw_call(ctx, idx, plain) == (RK_ERR_UNSUPPORTED, True) and b"counts" in last()   # queries without counts: nothing is written
    with pytest.raises(capi.RkError) as e:
        ctx.screen_abund_rows(idx, plain)
    assert e.value.code == RK_ERR_UNSUPPORTED
    assert raw_call(ctx, idx, qs, (0, 0, 0, 0, 0)) == (RK_ERR_ARG, True) and b"min_common" in last()
    assert raw_call(ctx, idx, qs, None) == (RK_ERR_ARG, True)
    for skip in (1, 2, 4, 5, 6, 7, 8, 9, 10, 11):   # idx, queries, off_out, recs_out, abund_out, n_recs, matched_out, n_cand_out, claimed_out, occ_out
        assert raw_call(ctx, idx, qs, skip=skip) == (RK_ERR_ARG, True), skip
    wrefs, wqd, wbits, _ = clade_case(True)
    assert raw_call(ctx, idx, counted(ctx, wqd, True)) == (RK_ERR_ARG, True) and b"widths" in last()
    assert raw_call(ctx, index_of(ctx, wrefs, True, wbits), qs) == (RK_ERR_ARG, True) and b"widths" in last()
    twice = ctx.sketches_from_host(np.array([5, 5, 9], dtype=np.uint32), np.array([0, 3], dtype=np.uint64))   # references that repeat a hash
    assert raw_call(ctx, ctx.index_build(twice, 24), qs) == (RK_ERR_UNSUPPORTED, True) and b"sets" in last()
    sk = ctx.sketches_from_host(*csr(refs[:200]))   # one hash range of a sharded build carries no complete posting lists
    assert raw_call(ctx, ctx.index_build_shard(sk, bits, 0, 2), qs) == (RK_ERR_ARG, True) and b"posting lists" in last()
    with pytest.raises(ValueError):
        ctx.screen_abund_rows(idx, qs, out=(np.zeros(3, dtype=np.uint32),) * 4)
    assert raw_call(ctx, idx, qs)[0] == 0   # and the good call runs (its records are the library's: leaked here, a few KB)


# ---- 8. the tool --------------------------------------------------------------------------------------------------------------------------
def run_tool(cwd, args):
    return subprocess.run([TOOL, "screen"] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_tool_screen_abund(ctx, tmp_path):
    rnames, refs, qnames, queries, triples = golden_pair("32")
    for name in ("ref.sketch", "qry.sketch"):
        shutil.copy(os.path.join(GOLDEN, "dist", name), tmp_path / name)
    shutil.copy(os.path.join(GOLDEN, "dist", "ref.sketch"), tmp_path / "host.sketch")
    qd = seeded_counts(queries, 77)
    ar.write_abund(tmp_path / "qry.sketch.abund", [len(q) for q in queries], [qd[i][int(h)] for i, q in enumerate(queries) for h in q])   # in the file's order
    idx, qs = index_of(ctx, refs), counted(ctx, qd)
    for extra, min_common, min_won in (([], 1, 0), (["--min-common", "5", "--min-won", "1"], 5, 1)):
        p = run_tool(tmp_path, ["-r", "ref.sketch", "-q", "qry.sketch", "--abund", "-o", "out.txt", "--summary", "sum.txt"] + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        (off, recs, abund, matched, n_cand, claimed, occ), st = screened(ctx, idx, qs, refs, qd, min_common, min_won)
        lines = (tmp_path / "out.txt").read_text().splitlines()
        assert len(lines) == len(recs) >= 5
        for line, r, a in zip(lines, recs, abund):
            f = line.split("\t")
            assert len(f) == 11 and f[:5] == [qnames[r["query"]], rnames[r["ref"]], str(r["common"]), str(r["size_ref"]), str(r["won"])]
            assert f[7:] == [str(a["med_common"]), "%.3f" % (int(a["occ_common"]) / int(r["common"])), str(a["med_won"]),
                             "%.3f" % (int(a["occ_won"]) / int(r["won"]) if r["won"] else 0.0)]
        assert (tmp_path / "sum.txt").read_text().splitlines() == [
            "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % (qnames[q], len(queries[q]), matched[q], n_cand[q], claimed[q], off[q + 1] - off[q], occ[q][0], occ[q][1], occ[q][2])
            for q in range(len(queries))]
        # without --abund: today's output, the first seven columns of the lines above and the first six of the summary
        p = run_tool(tmp_path, ["-r", "ref.sketch", "-q", "qry.sketch", "-o", "plain.txt", "--summary", "plainsum.txt"] + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert (tmp_path / "plain.txt").read_text().splitlines() == ["\t".join(line.split("\t")[:7]) for line in lines]
        assert (tmp_path / "plainsum.txt").read_text().splitlines() == ["\t".join(x.split("\t")[:6]) for x in (tmp_path / "sum.txt").read_text().splitlines()]
    # --sub: the counts survive the removal of the host -- here the references themselves, so only unindexed hashes stay, with their counts
    p = run_tool(tmp_path, ["-r", "ref.sketch", "-q", "qry.sketch", "--abund", "--sub", "host.sketch", "-o", "sub.txt", "--summary", "subsum.txt"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    left, _ = ctx.sketches_mask_counts(qs, idx, 0, 0)
    off, recs, abund, matched, n_cand, claimed, occ, st = ctx.screen_abund_rows(idx, left)
    sizes = np.diff(left.download()[1]).tolist()
    held = set(int(h) for r in refs for h in r)
    assert occ[:, 0].tolist() == [sum(c for h, c in m.items() if h not in held) for m in qd] and max(sizes) > 0 and len(recs) == 0
    assert (tmp_path / "sub.txt").read_text() == ""
    assert (tmp_path / "subsum.txt").read_text().splitlines() == ["%s\t%d\t0\t0\t0\t0\t%d\t0\t0" % (qnames[q], sizes[q], occ[q][0]) for q in range(len(queries))]
    # what dies, with a message, before a file is written: no side-car; a side-car of other sketches; sequence files as queries
    ar.write_abund(tmp_path / "qry.sketch.abund", [len(q) + 1 for q in queries], [1] * (sum(len(q) for q in queries) + len(queries)))
    p = run_tool(tmp_path, ["-r", "ref.sketch", "-q", "qry.sketch", "--abund", "-o", "x.txt"])
    assert p.returncode != 0 and b"qry.sketch.abund" in p.stderr and b"size differs" in p.stderr and not (tmp_path / "x.txt").exists()
    os.remove(tmp_path / "qry.sketch.abund")
    p = run_tool(tmp_path, ["-r", "ref.sketch", "-q", "qry.sketch", "--abund", "-o", "x.txt"])
    assert p.returncode != 0 and b"--abund needs the occurrence counts" in p.stderr and b"qry.sketch.abund" in p.stderr and not (tmp_path / "x.txt").exists()
    (tmp_path / "q.list").write_text("nothing.fa\n")
    p = run_tool(tmp_path, ["-r", "ref.sketch", "-q", "q.list", "--abund", "-o", "x.txt"])
    assert p.returncode != 0 and b"--abund needs -q x.sketch" in p.stderr and not (tmp_path / "x.txt").exists()
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"[--abund] -o out [--summary FILE]" in p.stderr
