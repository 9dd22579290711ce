"""rk_screen_rows on the device against tests/_screen_ref.py: the real reference's intersection counts on the golden pairs, random clades
under every option and both hash widths, the three walks of the winner pass at their seams with the winner first, in the middle and last
(read from the call's stats which walk ran), ties under every caller order, a species whose every hash goes to one strain under both
variants of the add, tiles and sketch boundaries, the emission in chunks, batches, row shards, the host leg, the cross-checks against
rk_dist_rows, rk_gather_rows and rk_group_sketches, the refusals and `rabbit_kssd screen`.  Every comparison is exact but the two printed
identities of the tool."""
import ctypes as C
import itertools
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _screen_ref as sr
from _selfjoin_cases import TOOL, csr, device_index
from conftest import GOLDEN
from rabbitkssd_amd import capi
from _screen_cases import ROWS_ARGTYPES, clades, golden_pair, imported_index, index_of, queries_of

pytestmark = pytest.mark.gpu
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def list_lengths(refs, queries, rows):
    lists = sr.posting_lists(refs)
    return [len(lists[h]) for q in rows for h in set(int(x) for x in queries[q]) if h in lists]


def screened(ctx, idx, qs, refs, queries, min_common=1, min_won=0, path=1, want=None, **rows):
    """the call, with what every result must satisfy, compared exactly with the reference; returns (arrays, stats)"""
    got = ctx.screen_rows(idx, qs, min_common, min_won, **rows)
    off, recs, matched, n_cand, claimed, st = got
    sel = sr.selected_rows(len(queries), rows.get("row_first", 0), rows.get("row_step", 1), rows.get("row_block", 0))
    result = want if want is not None else sr.fast(refs, queries, min_common, min_won)
    w_off, w_recs, w_matched, w_cand, w_claimed = sr.as_arrays(result, refs, queries, sel)
    assert st["path"] == path and st["rows"] == len(sel)
    assert off.tolist() == w_off and sr.rec_tuples(recs) == w_recs
    assert matched.tolist() == w_matched and n_cand.tolist() == w_cand and claimed.tolist() == w_claimed
    assert (st["lane_max"], st["wave_max"], st["tile_hashes"], st["threads"]) == CONSTANTS.setdefault("c", (st["lane_max"], st["wave_max"], st["tile_hashes"], st["threads"]))
    if not len(sel) or not len(refs):
        assert st["batches"] == 0 and st["launches"] == 0 and st["read_backs"] == 0
        return got[:5], st
    assert st["records"] == len(w_recs) and st["matched"] == sum(w_matched) and st["candidates"] == sum(w_cand) and st["claimed"] == sum(w_claimed)
    lens = list_lengths(refs, queries, sel)
    assert st["postings_walked"] == sum(lens)
    assert st["lane_lists"] == sum(n <= st["lane_max"] for n in lens) and st["wave_lists"] == sum(st["lane_max"] < n <= st["wave_max"] for n in lens)
    assert st["block_lists"] == sum(n > st["wave_max"] for n in lens)
    if path == 1:
        assert 1 <= st["rows_per_batch"] <= len(sel) and st["batches"] == -(-len(sel) // st["rows_per_batch"]) == st["read_backs"]
        assert 2 * st["batches"] + 2 <= st["launches"] <= 4 * st["batches"] + 2 and st["adds"] <= st["claimed"]
    else:
        assert st["batches"] == 1 and st["launches"] == 0 and st["adds"] == 0 and st["read_backs"] == 0
    if min_common == 1:
        assert claimed.tolist() == matched.tolist()
    return got[:5], st


CONSTANTS = {}


def constants(ctx):
    one = [np.array([1], dtype=np.uint32)]
    st = ctx.screen_rows(index_of(ctx, one), queries_of(ctx, one))[5]
    return st["lane_max"], st["wave_max"], st["tile_hashes"], st["threads"]


def result_bytes(arrays):
    return b"".join(a.tobytes() for a in arrays)


# ---- 1. the real reference's intersection counts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,how", [("32", "built"), ("32", "imported"), ("64", "built"), ("64", "imported")])
def test_golden_pairs_carry_the_references_own_counts(ctx, tag, how):
    rnames, refs, qnames, queries, triples = golden_pair(tag)
    wide, bits = (True, 36) if tag == "64" else (False, 24)
    idx = (index_of if how == "built" else imported_index)(ctx, refs, wide, bits)
    qs = queries_of(ctx, queries, wide)
    for min_common, min_won in ((1, 0), (5, 1)):
        (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, qs, refs, queries, min_common, min_won)
        assert st["batches"] == 1 and len(recs) >= 1
        for p in recs:   # the real reference's intersection count and sizes of that pair
            assert (int(p["common"]), int(p["size_ref"]), int(p["size_query"])) == triples[(qnames[p["query"]], rnames[p["ref"]])]
        for q in range(len(queries)):
            assert n_cand[q] == sum(triples[(qnames[q], r)][0] >= min_common for r in rnames)


# ---- 2. random clades, every option, both widths -------------------------------------------------------------------------------------
_wanted = {}


def wanted(wide, min_common, min_won):
    """the reference's answer on clades(wide), computed once and shared"""
    key = (wide, min_common, min_won)
    if key not in _wanted:
        refs, queries, bits = clades(wide)
        _wanted[key] = sr.fast(refs, queries, min_common, min_won)
    return _wanted[key]


@pytest.mark.parametrize("wide", [False, True])
def test_random_clades_under_every_option(ctx, wide):
    refs, queries, bits = clades(wide)
    idx = index_of(ctx, refs, wide, bits)
    assert not np.array_equal(idx.order, np.arange(len(refs)))   # internal order != caller order
    qs = queries_of(ctx, queries, wide)
    for min_common in (1, 2, 5):
        for min_won in (0, 1, 3):
            arrays, st = screened(ctx, idx, qs, refs, queries, min_common, min_won, want=wanted(wide, min_common, min_won))
            assert st["batches"] == 1
    sr.facts(refs, queries, wanted(wide, 1, 0))
    a, _ = screened(ctx, idx, qs, refs, queries, want=wanted(wide, 1, 0))
    b, _ = screened(ctx, imported_index(ctx, refs, wide, bits), qs, refs, queries, want=wanted(wide, 1, 0))
    assert result_bytes(a) == result_bytes(b)   # built and imported: the same bytes


# ---- 3. the walks at their seams ------------------------------------------------------------------------------------------------------
N_SEAM, FIRST_CHAMPION = 3300, 1600


def seam_collection(lane_max, wave_max, threads):
    """One shared hash per (length, position): its champion -- a reference whose every hash is in the query, so nobody beats it -- and
    length - 1 fillers (8 hashes outside the query each: containment below 1) with smaller or larger indices so that the champion is the
    first, a middle or the last posting of the list of an index in the caller's order.  Then a list whose LAST posting is its only
    candidate at min_common = 2, and a list without any."""
    lengths = sorted({n + d for n in (lane_max, wave_max, 64, 128, wave_max + threads, wave_max + 2 * threads) for d in (-1, 0, 1)})
    rng = np.random.default_rng(12)
    pool = rng.permutation(1 << 22).astype(np.uint32)
    take = iter(pool.tolist())
    parts = [[] for _ in range(N_SEAM)]
    query, champion, plan = [], FIRST_CHAMPION, []
    for n in lengths:
        for where in ("first", "middle", "last"):
            below = {"first": 0, "middle": (n - 1) // 2, "last": n - 1}[where]
            lo = rng.choice(FIRST_CHAMPION, size=below, replace=False)
            hi = FIRST_CHAMPION + 100 + rng.choice(N_SEAM - FIRST_CHAMPION - 100, size=n - 1 - below, replace=False)
            s = next(take)
            for v in [champion] + lo.tolist() + hi.tolist():
                parts[v].append(s)
            query.append(s)
            plan.append((s, n, where, champion))
            champion += 1
    assert champion <= FIRST_CHAMPION + 90
    fillers = [v for v in range(N_SEAM) if not FIRST_CHAMPION <= v < FIRST_CHAMPION + 100]
    for v in fillers:
        parts[v] += [next(take) for _ in range(8)]
    # singles: references FIRST_CHAMPION + 90 .. + 97 hold one query hash each (common 1) but for the last of the first list, which holds two
    only_last, nobody, extra = next(take), next(take), next(take)
    for v in range(FIRST_CHAMPION + 90, FIRST_CHAMPION + 94):
        parts[v].append(only_last)
    parts[FIRST_CHAMPION + 93].append(extra)
    for v in range(FIRST_CHAMPION + 94, FIRST_CHAMPION + 98):
        parts[v].append(nobody)
    query += [only_last, nobody, extra]
    refs = [np.sort(np.array(p, dtype=np.uint32)) for p in parts]
    return refs, np.sort(np.array(query, dtype=np.uint32)), plan, lengths, (only_last, nobody, FIRST_CHAMPION + 93)


@pytest.mark.parametrize("how", ["imported", "built"])
def test_every_walk_of_the_winner_pass_at_its_seams(ctx, how):
    lane_max, wave_max, tile, threads = constants(ctx)
    assert 1 <= lane_max < 63 and 129 < wave_max and wave_max % 64 == 0 and wave_max + 2 * threads + 1 < FIRST_CHAMPION
    refs, query, plan, lengths, (only_last, nobody, last_holder) = seam_collection(lane_max, wave_max, threads)
    idx = (imported_index if how == "imported" else index_of)(ctx, [r for r in refs], False, 24)
    qs = queries_of(ctx, [query])
    want = sr.fast(refs, [query])
    won = {r: w for _, r, c, w in want[0][0]}
    # A list ascends in INTERNAL genome id, and the plan places the champion in the caller's order: on the imported index (the identity)
    # the champion is the first, the middle or the last posting of every list, whichever walk takes it; the build renumbers, so there the
    # winner sits wherever the internal order puts it (computed, not controlled: the result must not care)
    lists = sr.posting_lists(refs)
    order = idx.order
    inv = np.empty(N_SEAM, dtype=np.int64)
    inv[order] = np.arange(N_SEAM)
    if how == "imported":
        assert np.array_equal(order, np.arange(N_SEAM))
    for s, n, where, champion in plan:
        holders = sorted(int(inv[v]) for v in lists[int(s)])
        assert won[champion] == 1 and len(holders) == n
        if how == "imported":
            assert holders.index(int(inv[champion])) == {"first": 0, "middle": (n - 1) // 2, "last": n - 1}[where]
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, qs, refs, [query], want=want)
    assert st["lane_lists"] == 3 * sum(n <= lane_max for n in lengths) + 3 and st["wave_lists"] == 3 * sum(lane_max < n <= wave_max for n in lengths)
    assert st["block_lists"] == 3 * sum(n > wave_max for n in lengths) >= 21
    assert sum(int(r["won"]) for r in recs if FIRST_CHAMPION <= r["ref"] < FIRST_CHAMPION + 90) == len(plan)
    # min_common = 2: the singles are no candidates; `only_last` goes to its last holder, `nobody` is unclaimed
    want2 = sr.fast(refs, [query], 2)
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, qs, refs, [query], 2, want=want2)
    by_ref = {int(r["ref"]): int(r["won"]) for r in recs}
    assert by_ref[last_holder] == 2 and all(v not in by_ref for v in range(FIRST_CHAMPION + 94, FIRST_CHAMPION + 98)) and claimed[0] < matched[0]


# ---- 4. ties --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["built", "imported"])
def test_ties_go_by_size_then_by_the_callers_index_under_every_order(ctx, how):
    pool = np.random.default_rng(4).permutation(1 << 22)[:400].astype(np.uint32)
    shared, query = pool[0], np.sort(pool[0:4])
    # equal ratios from different counts: 2 of 4, 3 of 6, 1 of 2, all hold `shared`
    X = [pool[0], pool[1], pool[50], pool[51]]
    Y = [pool[0], pool[2], pool[3], pool[60], pool[61], pool[62]]
    Z = [pool[0], pool[70]]
    # equal ratio and size: 2 of 4 each, all hold `shared`
    P, Q, R = [pool[0], pool[1], pool[80], pool[81]], [pool[0], pool[2], pool[90], pool[91]], [pool[0], pool[3], pool[100], pool[101]]
    make = index_of if how == "built" else (lambda c, parts: imported_index(c, parts, False, 24))
    extra = [np.sort(pool[350 + 5 * k: 355 + 5 * k]) for k in range(3)]   # bystanders, so that the build has something to renumber
    for roles in ((X, Y, Z), (P, Q, R)):
        for order in itertools.permutations(range(3)):   # role k sits at caller index order[k]: lists hold internal ids, the tie goes by the caller's
            refs = [None] * 3
            for role, at in zip(roles, order):
                refs[at] = np.sort(np.array(role, dtype=np.uint32))
            refs = refs + extra
            (off, recs, matched, n_cand, claimed), st = screened(ctx, make(ctx, refs), queries_of(ctx, [query]), refs, [query])
            won = {int(r["ref"]): int(r["won"]) for r in recs}
            if roles[0] is X:
                assert won == {order[0]: 1, order[1]: 3, order[2]: 0}       # the largest of the three halves takes the shared hash
            else:
                assert won == {0: 2, 1: 1, 2: 1}                             # the smallest caller's index takes it
    assert shared in query


# ---- 5. contention and the combine ----------------------------------------------------------------------------------------------------
def test_a_species_whose_superset_strain_wins_everything_under_both_adds(ctx, monkeypatch):
    rng = np.random.default_rng(8)
    pool = rng.permutation(1 << 23)[:4000].astype(np.uint32)
    core = pool[:100]
    strains = [np.sort(np.concatenate([core, pool[100 + 10 * v: 110 + 10 * v]])) for v in range(300)]
    hub = 137
    strains[hub] = np.sort(pool[:100 + 10 * 300])   # holds what every strain holds
    query = strains[hub]
    idx, qs = index_of(ctx, strains), queries_of(ctx, [query])
    want = sr.fast(strains, [query])
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, qs, strains, [query], want=want)
    assert len(recs) == 300 and int(recs[hub]["won"]) == len(query) == 3100 and all(int(r["won"]) == 0 for r in recs if r["ref"] != hub)
    assert st["adds"] * 8 < st["claimed"] and st["wave_lists"] == 100      # one address: the waves combine
    monkeypatch.setenv("RK_SCREEN_COMBINE", "0")
    plain, st0 = screened(ctx, idx, qs, strains, [query], want=want)
    monkeypatch.delenv("RK_SCREEN_COMBINE")
    assert st0["adds"] == st0["claimed"] == 3100 and result_bytes(plain) == result_bytes((off, recs, matched, n_cand, claimed))
    refs, queries, bits = clades(False)   # and on a collection with many winners
    idx, qs = index_of(ctx, refs, False, bits), queries_of(ctx, queries)
    a, sa = screened(ctx, idx, qs, refs, queries, want=wanted(False, 1, 0))
    monkeypatch.setenv("RK_SCREEN_COMBINE", "0")
    b, sb = screened(ctx, idx, qs, refs, queries, want=wanted(False, 1, 0))
    monkeypatch.delenv("RK_SCREEN_COMBINE")
    assert result_bytes(a) == result_bytes(b) and sa["adds"] < sb["adds"] == sb["claimed"]


# ---- 6. tiles and rows ----------------------------------------------------------------------------------------------------------------
def test_sketch_boundaries_around_tiles_and_lane_seams(ctx):
    lane_max, wave_max, tile, threads = constants(ctx)
    rng = np.random.default_rng(15)
    pool = rng.permutation(1 << 23).astype(np.uint32)
    universe, foreign = pool[:6000], pool[6000:12000]
    refs = [np.sort(rng.choice(universe, size=int(rng.integers(100, 400)), replace=False)) for _ in range(40)]
    indexed = np.unique(np.concatenate(refs))
    # the sketches end at 63, 64, 65, then three empty ones, at tile - 1, tile, tile + 1, tile + 2, three empty ones, 2 tile, 2 tile + 1, ..
    sizes = [63, 1, 1, 0, 0, 0, tile - 66, 1, 1, 1, 0, 0, 0, tile - 2, 1, 1, 2 * tile, 5, 0]
    ends = np.cumsum(sizes).tolist()
    assert {63, 64, 65, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1}.issubset(ends) and ends[-1] > 4 * tile
    queries = []
    for k, n in enumerate(sizes):
        src = indexed if k % 3 == 0 else foreign if k % 3 == 1 else np.concatenate([indexed[:3000], foreign[:3000]])
        queries.append(np.sort(rng.choice(src, size=n, replace=False)).astype(np.uint32))
    queries[16] = np.sort(rng.choice(indexed, size=2 * tile, replace=False)).astype(np.uint32)      # every hash matches
    queries[13] = np.sort(rng.choice(foreign, size=tile - 2, replace=False)).astype(np.uint32)      # no hash matches
    idx = index_of(ctx, refs)
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, queries_of(ctx, queries), refs, queries)
    assert matched[16] == 2 * tile and matched[13] == 0 and n_cand[13] == 0 and off[14] == off[13]
    for shift in (1, 62, tile - 63):   # the same sketches behind a first one that moves every boundary
        moved = [np.sort(rng.choice(indexed, size=shift, replace=False)).astype(np.uint32)] + queries
        screened(ctx, idx, queries_of(ctx, moved), refs, moved)
    for qset in ([queries[3]], [queries[3]] * 5, [queries[13]], [queries[3], queries[16], queries[3]]):   # empty sketches only; no match at all
        screened(ctx, idx, queries_of(ctx, qset), refs, qset)


# ---- 7. the emission -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 513])
def test_more_candidates_than_one_chunk_of_the_write_kernel(ctx, n):
    threads = constants(ctx)[3]
    assert threads < n
    pool = np.random.default_rng(22).permutation(1 << 22).astype(np.uint32)
    # every reference holds the shared hash and two of its own; the query holds the shared hash and one of each reference's own: all are
    # candidates.  Every third reference (but the first) holds nothing of its own in the query: its only hash goes to a better one
    refs = [np.sort(np.concatenate([pool[:1], pool[1 + 2 * v: 3 + 2 * v]])) for v in range(n)]
    query = np.sort(np.concatenate([pool[:1]] + [pool[1 + 2 * v: 2 + 2 * v] for v in range(n) if v % 3 != 2]))
    idx, qs = index_of(ctx, refs), queries_of(ctx, [query])
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, qs, refs, [query])
    assert n_cand.tolist() == [n] and recs["ref"].tolist() == list(range(n)) and st["wave_lists"] + st["block_lists"] == 1
    assert recs["won"].tolist() == [2] + [0 if v % 3 == 2 else 1 for v in range(1, n)]
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, qs, refs, [query], 1, 1)   # records cut out of the middle of every chunk
    assert recs["ref"].tolist() == [v for v in range(n) if v % 3 != 2] and n_cand.tolist() == [n]
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, qs, refs, [query], 1, 2)
    assert recs["ref"].tolist() == [0]
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, qs, refs, [query], 1, 3)   # every record is filtered
    assert len(recs) == 0 and off.tolist() == [0, 0] and n_cand.tolist() == [n] and claimed.tolist() == matched.tolist()


# ---- 8. batches, shards, the host leg ---------------------------------------------------------------------------------------------------
def test_three_batches_of_seven_rows_give_the_bytes_of_one(ctx, monkeypatch):
    refs, queries, bits = clades(False)
    queries, want = queries[:7], wanted(False, 1, 0)[:7]
    idx, qs = index_of(ctx, refs, False, bits), queries_of(ctx, queries)
    whole, st = screened(ctx, idx, qs, refs, queries, want=want)
    assert st["batches"] == 1 and st["rows_per_batch"] == 7
    row_bytes = 8 * len(refs) + 16   # rk_screen.hip: the counter row and the won row
    monkeypatch.setenv("RK_SCREEN_BATCH_BYTES", str(3 * row_bytes + row_bytes // 2))
    some, st = screened(ctx, idx, qs, refs, queries, want=want)
    assert st["rows_per_batch"] == 3 and st["batches"] == 3 and result_bytes(some) == result_bytes(whole)
    monkeypatch.setenv("RK_SCREEN_BATCH_BYTES", "1")   # less than a row: one row per batch
    single, st = screened(ctx, idx, qs, refs, queries, 2, 1, want=wanted(False, 2, 1)[:7])
    assert st["batches"] == 7 and st["rows_per_batch"] == 1
    shard, st = screened(ctx, idx, qs, refs, queries, want=want, row_first=1, row_step=2, row_block=1)   # rows 1 3 5, one per batch
    assert st["batches"] == 3
    monkeypatch.delenv("RK_SCREEN_BATCH_BYTES")


@pytest.mark.parametrize("block", [1, 3])
def test_row_shards_concatenate_to_the_whole(ctx, block):
    refs, queries, bits = clades(False)
    idx, qs = index_of(ctx, refs, False, bits), queries_of(ctx, queries)
    want = wanted(False, 2, 1)
    whole, _ = screened(ctx, idx, qs, refs, queries, 2, 1, want=want)
    out = tuple(np.full(len(queries), 0xDEAD, dtype=np.uint32) for _ in range(3))
    parts = []
    for first in (0, 1, 2):
        (off, recs, m, c, v), st = screened(ctx, idx, qs, refs, queries, 2, 1, want=want, row_first=first, row_step=3, row_block=block)
        parts.append(recs)
        rows = sr.selected_rows(len(queries), first, 3, block)
        before = [a.copy() for a in out]
        got = ctx.screen_rows(idx, qs, 2, 1, row_first=first, row_step=3, row_block=block, out=out)   # one set of arrays for the shards
        assert all(a is b for a, b in zip(got[2:5], out))
        for a, b in zip(out, before):   # unselected entries are untouched
            assert all(a[q] == b[q] for q in range(len(queries)) if q not in rows)
    both = np.concatenate(parts)
    both = both[np.lexsort((both["ref"], both["query"]))]
    assert both.tobytes() == whole[1].tobytes() and all(np.array_equal(a, b) for a, b in zip(out, whole[2:]))


def test_host_leg_gives_the_same_bytes(ctx, monkeypatch):
    for wide in (False, True):
        refs, queries, bits = clades(wide)
        qs = queries_of(ctx, queries, wide)
        for make in (index_of, imported_index):
            idx = make(ctx, refs, wide, bits)
            for min_common, min_won in ((1, 0), (2, 1)):
                device, st = screened(ctx, idx, qs, refs, queries, min_common, min_won, want=wanted(wide, min_common, min_won))
                monkeypatch.setenv("RK_SCREEN_DEVICE", "0")
                host, st2 = screened(ctx, idx, qs, refs, queries, min_common, min_won, path=2, want=wanted(wide, min_common, min_won))
                screened(ctx, idx, qs, refs, queries, min_common, min_won, path=2, want=wanted(wide, min_common, min_won), row_first=1, row_step=2, row_block=3)
                monkeypatch.delenv("RK_SCREEN_DEVICE")
                assert result_bytes(host) == result_bytes(device)
                same = ("records", "candidates", "matched", "claimed", "rows", "postings_walked", "lane_lists", "wave_lists", "block_lists")
                assert {k: st2[k] for k in same} == {k: st[k] for k in same}


def test_timed_span(ctx, monkeypatch):
    refs, queries, bits = clades(False)
    idx, qs = index_of(ctx, refs, False, bits), queries_of(ctx, queries)
    ctx.set_timing(True)
    screened(ctx, idx, qs, refs, queries, want=wanted(False, 1, 0))
    assert ctx.last_ms(capi.MS_SCREEN) > 0.0
    monkeypatch.setenv("RK_SCREEN_DEVICE", "0")
    screened(ctx, idx, qs, refs, queries, path=2, want=wanted(False, 1, 0))
    monkeypatch.delenv("RK_SCREEN_DEVICE")
    assert ctx.last_ms(capi.MS_SCREEN) == 0.0
    ctx.set_timing(False)


# ---- 9. cross-checks inside the project -----------------------------------------------------------------------------------------------
def test_common_is_the_count_of_dist_rows(ctx):
    refs, queries, bits = clades(False)
    idx, qs = index_of(ctx, refs, False, bits), queries_of(ctx, queries)
    dense = ctx.dist_rows(idx, qs, 0, 0, 20, 1.0, want_dense=True)[1]
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, qs, refs, queries, 2, 0, want=wanted(False, 2, 0))
    assert len(recs) > 100 and all(int(dense[r["query"], r["ref"]]) == int(r["common"]) for r in recs)
    assert n_cand.tolist() == (dense >= 2).sum(axis=1).tolist()


def test_equal_sized_references_best_record_is_gathers_first_pick(ctx):
    rng = np.random.default_rng(33)
    pool = rng.permutation(1 << 22)[:3000].astype(np.uint32)
    refs = [np.sort(rng.choice(pool, size=60, replace=False)) for _ in range(200)]   # one size
    queries = [np.sort(np.unique(np.concatenate([refs[a][:40], refs[b][:50], refs[c]]))) for a, b, c in rng.integers(0, 200, size=(12, 3))]
    idx, qs = index_of(ctx, refs), queries_of(ctx, queries)
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, qs, refs, queries)
    g_off, picks, g_matched, g_cand, covered, gst = ctx.gather_rows(idx, qs, 1, 1)
    assert matched.tolist() == g_matched.tolist() and n_cand.tolist() == g_cand.tolist() and len(picks) == len(queries)
    for q in range(len(queries)):
        mine = recs[int(off[q]):int(off[q + 1])]
        best = max(mine, key=lambda r: (int(r["common"]), -int(r["ref"])))
        assert (int(best["ref"]), int(best["won"]), int(best["common"])) == (int(picks[q]["ref"]), int(picks[q]["fresh"]), int(picks[q]["common"]))
        assert best["won"] == best["common"]


def test_a_pan_sketch_is_claimed_entirely_by_its_own_collection(ctx):
    refs, _, bits = clades(False)
    idx = index_of(ctx, refs, False, bits)
    labels = [(v * 7919) % len(refs) // 125 * 125 for v in range(len(refs))]   # 8 groups of 125 genomes
    sk, gl, gs, gst = ctx.group_sketches(idx, labels, "pan")
    h, off = sk.download()
    pans = sr.parts_of(h, off)
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, sk, refs, pans)
    assert matched.tolist() == claimed.tolist() == [len(p) for p in pans] and min(matched) > 1000
    for q in range(8):   # the best candidate keeps everything it shares
        mine = recs[int(off[q]):int(off[q + 1])]
        key = lambda r: (Fraction(int(r["common"]), int(r["size_ref"])), int(r["size_ref"]), -int(r["ref"]))   # noqa: E731
        best = max(mine, key=key)
        assert best["won"] == best["common"] and mine["won"].sum() == len(pans[q])


# ---- 10. the empty cases and what is refused ---------------------------------------------------------------------------------------------
def test_empty_cases(ctx):
    refs, queries, bits = clades(False)
    idx = index_of(ctx, refs, False, bits)
    # Q = 0: nothing runs
    none_q = ctx.sketches_from_host(np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64))
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, none_q, refs, [], path=0)
    assert off.tolist() == [0] and len(recs) == len(matched) == 0 and st["path"] == 0
    # an index without genomes: every row empty
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 24)
    qset = [refs[0], queries[-2]]
    (off, recs, matched, n_cand, claimed), st = screened(ctx, none, queries_of(ctx, qset), [], qset, path=0)
    assert off.tolist() == [0, 0, 0] and len(recs) == 0 and matched.tolist() == [0, 0] and st["rows"] == 2
    # a row shard that selects nothing
    (off, recs, matched, n_cand, claimed), st = screened(ctx, idx, queries_of(ctx, qset), refs, qset, path=0, row_first=5, row_step=7, row_block=1)
    assert off.tolist() == [0, 0, 0] and st["rows"] == 0


def raw_call(ctx, idx, qs, opts=(1, 0, 0, 0, 0), skip=None):
    L = capi.lib()
    L.rk_screen_rows.argtypes = ROWS_ARGTYPES
    q = qs.count if qs is not None else 2
    off = np.full(q + 1, 0x77, dtype=np.uint64)
    outs = [np.full(q, 0x55, dtype=np.uint32) for _ in range(3)]
    recs, n = C.c_void_p(0x1234), C.c_uint64(0xABAB)
    o = capi.ScreenOpts(*opts) if opts is not None else None
    args = [ctx._h, idx._h if idx is not None else None, qs._h if qs is not None else None, C.byref(o) if o is not None else None, off.ctypes.data,
            C.byref(recs), C.byref(n), outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, C.byref(capi.ScreenStats())]
    if skip is not None:
        args[skip] = None
    rc = L.rk_screen_rows(*args)
    return rc, recs.value == 0x1234 and n.value == 0xABAB and bool((off == 0x77).all()) and all(bool((a == 0x55).all()) for a in outs)


def test_arguments_that_are_refused(ctx):
    refs, queries, bits = clades(False)
    idx, qs = index_of(ctx, refs, False, bits), queries_of(ctx, queries)
    last = lambda: capi.lib().rk_last_error(ctx._h)   # noqa: E731
    assert raw_call(ctx, idx, qs, (0, 0, 0, 0, 0)) == (RK_ERR_ARG, True) and b"min_common" in last()
    assert raw_call(ctx, idx, qs, None) == (RK_ERR_ARG, True)
    for skip in (1, 2, 4, 5, 6, 7, 8, 9):   # idx, queries, off_out, recs_out, n_recs, matched_out, n_cand_out, claimed_out
        assert raw_call(ctx, idx, qs, skip=skip) == (RK_ERR_ARG, True), skip
    wrefs, wqueries, wbits = clades(True)
    assert raw_call(ctx, idx, queries_of(ctx, wqueries, True)) == (RK_ERR_ARG, True) and b"widths" in last()
    assert raw_call(ctx, index_of(ctx, wrefs, True, wbits), qs) == (RK_ERR_ARG, True) and b"widths" in last()
    # sketches that repeat a hash: queries, then references
    twice = ctx.sketches_from_host(np.array([5, 5, 9], dtype=np.uint32), np.array([0, 3], dtype=np.uint64))
    assert raw_call(ctx, idx, twice) == (RK_ERR_UNSUPPORTED, True) and b"sets" in last()
    assert raw_call(ctx, ctx.index_build(twice, 24), qs) == (RK_ERR_UNSUPPORTED, True) and b"sets" in last()
    # one hash range of a sharded build carries no complete posting lists
    sk = ctx.sketches_from_host(*csr(refs[:200]))
    assert raw_call(ctx, ctx.index_build_shard(sk, bits, 0, 2), qs) == (RK_ERR_ARG, True) and b"posting lists" in last()
    with pytest.raises(capi.RkError) as e:
        ctx.screen_rows(idx, qs, min_common=0)
    assert e.value.code == RK_ERR_ARG
    with pytest.raises(ValueError):
        ctx.screen_rows(idx, qs, out=(np.zeros(3, dtype=np.uint32),) * 3)
    assert raw_call(ctx, idx, qs)[0] == 0   # and the good call runs (its records are the library's: leaked here, a few KB)


def test_indexes_without_all_posting_lists_are_refused(ctx):
    import torch
    from rabbitkssd_amd import synth
    S = 2
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    sk = ctx.sketches_from_host(h, off)
    qs = queries_of(ctx, sr.parts_of(h, off)[:3])
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


# ---- 11. the tool -----------------------------------------------------------------------------------------------------------------------
def run_tool(cwd, args):
    return subprocess.run([TOOL, "screen"] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_tool_screen_subcommand(ctx, tmp_path):
    rnames, refs, qnames, queries, triples = golden_pair("32")
    shutil.copy(os.path.join(GOLDEN, "dist", "ref.sketch"), tmp_path / "ref.sketch")
    shutil.copy(os.path.join(GOLDEN, "dist", "qry.sketch"), tmp_path / "qry.sketch")
    K = None
    for line in open(os.path.join(GOLDEN, "dist", "dist_M0_D1_N0.ref.txt")):   # the k-mer length from a distance the real reference printed
        f = line.rstrip("\n").split("\t")
        c, s0, s1 = (int(x) for x in f[2].split("|"))
        j, d = float(f[3]), float(f[4])
        if 0 < c < min(s0, s1) and 0.0 < d < 1.0:
            K = round(-np.log(2 * j / (1 + j)) / d)
            break
    assert K in (16, 18, 20, 22, 24, 26, 28, 30, 32)
    idx, qs = index_of(ctx, refs), queries_of(ctx, queries)
    for extra, min_common, min_won in (([], 1, 0), (["--min-common", "5", "--min-won", "1"], 5, 1)):
        p = run_tool(tmp_path, ["-r", "ref.sketch", "-q", "qry.sketch", "-o", "out.txt", "--summary", "sum.txt"] + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        off, recs, matched, n_cand, claimed, st = ctx.screen_rows(idx, qs, min_common, min_won)
        assert len(recs) >= 5
        lines = (tmp_path / "out.txt").read_text().splitlines()
        assert len(lines) == len(recs)
        for line, r in zip(lines, recs):
            f = line.split("\t")
            assert f[:5] == [qnames[r["query"]], rnames[r["ref"]], str(r["common"]), str(r["size_ref"]), str(r["won"])]
            assert (int(f[2]), int(f[3])) == triples[(f[0], f[1])][:2]
            assert len(f) == 7 and all(len(x.split(".")[1]) == 6 for x in f[5:])
            # six decimals are printed: half a unit of the last place on either side
            assert abs(float(f[5]) - (int(r["common"]) / int(r["size_ref"])) ** (1 / K)) <= 1.0e-6
            assert abs(float(f[6]) - (int(r["won"]) / int(r["size_ref"])) ** (1 / K)) <= 1.0e-6
            assert f[6] == "0.000000" or r["won"] > 0
        assert (tmp_path / "sum.txt").read_text().splitlines() == ["%s\t%d\t%d\t%d\t%d\t%d" % (qnames[q], len(queries[q]), matched[q], n_cand[q], claimed[q], off[q + 1] - off[q])
                                                                   for q in range(len(queries))]
    # --sub: the queries lose the hashes of the --sub sketches first, exactly as masking through the API
    shutil.copy(os.path.join(GOLDEN, "dist", "qry.sketch"), tmp_path / "host.sketch")
    p = run_tool(tmp_path, ["-r", "ref.sketch", "-q", "qry.sketch", "--sub", "host.sketch", "-o", "sub.txt", "--summary", "subsum.txt"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    masked, _ = ctx.sketches_mask(qs, index_of(ctx, queries), 0, 0)
    off, recs, matched, n_cand, claimed, st = ctx.screen_rows(idx, masked, 1, 0)
    sizes = np.diff(masked.download()[1]).tolist()
    assert (tmp_path / "sub.txt").read_text().splitlines() == [] == [1 for _ in recs] and sizes == [0] * len(queries)   # a query minus itself
    assert (tmp_path / "subsum.txt").read_text().splitlines() == ["%s\t0\t0\t0\t0\t0" % qnames[q] for q in range(len(queries))]
    shutil.copy(os.path.join(GOLDEN, "dist", "ref.sketch"), tmp_path / "host.sketch")   # and minus the references: only unindexed hashes stay
    p = run_tool(tmp_path, ["-r", "ref.sketch", "-q", "qry.sketch", "--sub", "host.sketch", "-o", "sub.txt", "--summary", "subsum.txt"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    masked, _ = ctx.sketches_mask(qs, idx, 0, 0)
    off, recs, matched, n_cand, claimed, st = ctx.screen_rows(idx, masked, 1, 0)
    sizes = np.diff(masked.download()[1]).tolist()
    assert len(recs) == 0 and (tmp_path / "sub.txt").read_text() == "" and max(sizes) > 0
    assert (tmp_path / "subsum.txt").read_text().splitlines() == ["%s\t%d\t0\t0\t0\t0" % (qnames[q], sizes[q]) for q in range(len(queries))]
    # what dies, with a message, before a file is written
    for args, text in ((["-r", "ref.sketch", "-o", "x.txt"], b"needs -r and -q"), (["-q", "qry.sketch", "-o", "x.txt"], b"needs -r and -q"),
                       (["-r", "ref.sketch", "-q", "qry.sketch", "-o", "x.txt", "--gpus", "2"], b"one GPU"),
                       (["-r", "ref.sketch", "-q", "qry.sketch", "-o", "x.txt", "--min-common", "0"], b"--min-common must be >= 1")):
        p = run_tool(tmp_path, args)
        assert p.returncode != 0 and text in p.stderr and not (tmp_path / "x.txt").exists(), args
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"screen  -r" in p.stderr and b" convert screen merge " in p.stderr and b"p-value" in p.stderr
