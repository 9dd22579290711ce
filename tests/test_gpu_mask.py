"""rk_sketches_mask on the device against tests/_mask_ref.py: the real reference's own `sub` outputs on the golden pairs, the tiles, waves
and scan blocks at their seams (read from the call's stats, not copied), runs of empty sketches, keep patterns, the look-up at its
edges, the band at its edges, repeats on either side, 36-bit hashes, the result fed onward, the host leg, the refusals and the tool.
Every case asserts from the stats which leg ran and what it counted, then compares hashes and offsets exactly."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _mask_ref as mk
from _selfjoin_cases import KMER, TOOL, Oracle, csr, device_index
from conftest import GOLDEN
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth
from test_gpu_gather import gathered, queries_of
from test_gpu_group import imported_index, index_of
from test_mask_cpu import MASK_ARGTYPES, golden

pytestmark = pytest.mark.gpu
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6
BANDS = [mk.SUB, mk.PRESENT, (0, 1), (2, mk.MAX), (1, 2), (3, 3)]


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def masked(ctx, qs, idx, refs, queries, band, path=1):
    """the call, with what every result must satisfy, compared exactly with the reference over the queries as the device holds them
    (ascending); returns (survivors per query, stats, the object)"""
    sk, st = ctx.sketches_mask(qs, idx, *band)
    sorted_q = [sorted(np.asarray(q).tolist()) for q in queries]
    want = mk.from_counter(refs, sorted_q, *band)
    total = sum(len(q) for q in sorted_q)
    assert st["path"] == path and st["hashes"] == total and st["kept"] == sum(len(k) for k in want)
    assert st["matched"] == mk.matched(refs, sorted_q) and st["emptied"] == mk.emptied(sorted_q, want)
    assert st["tile_hashes"] >= 64 and st["threads"] >= 64 and st["tiles"] == -(-total // st["tile_hashes"])
    assert (st["scan_blocks"] >= 1) == (st["tiles"] >= 1)
    assert sk is not None and sk.count == len(queries) and sk.total == st["kept"] and sk.is64 == qs.is64 and sk.windows == 0
    h, off = sk.download()
    w_h, w_off = mk.as_arrays(want, np.uint64 if qs.is64 else np.uint32)
    assert h.dtype == w_h.dtype and np.array_equal(off, w_off) and np.array_equal(h, w_h)
    return want, st, sk


def tile_hashes(ctx):
    """T, from a first trivial call"""
    qs = queries_of(ctx, [np.array([1], dtype=np.uint32)])
    st = ctx.sketches_mask(qs, index_of(ctx, [np.array([2], dtype=np.uint32)]), 0, 0)[1]
    assert st["path"] == 1 and st["tiles"] == 1
    return st["tile_hashes"]


def scan_tiles(T):
    """the tiles one block of the scan takes: the geometry of the stats (the same on every leg), asked of the host rule"""
    for k in (1 << s for s in range(2, 16)):
        n = k * T + 1
        st = capi.mask_lists(np.zeros(n, dtype=np.uint32), [0, n], np.zeros(0, np.uint32), np.zeros(0, np.uint32))[2]
        assert st["tiles"] == k + 1
        if st["scan_blocks"] == 2:
            return k
    raise AssertionError("no scan seam below 2^15 tiles")


def runs(sizes, start=0):
    """sketches of consecutive integers: sketch i holds sizes[i] of them, the first begins at `start` -- the position of a hash is its value - start"""
    out, at = [], start
    for s in sizes:
        out.append(np.arange(at, at + s, dtype=np.uint32))
        at += s
    return out


def pattern_refs(name, total, T):
    """references over the hashes 0 .. total - 1 so that {0, 0} keeps: all, none, every other hash, or the even tiles only"""
    every = np.arange(total, dtype=np.uint32)
    if name == "all":
        return [np.array([total + 7], dtype=np.uint32)]
    if name == "none":
        return [every]
    if name == "alternating":
        return [every[every % 2 == 1]]
    assert name == "tiles"
    return [every[(every // T) % 2 == 1]]


PATTERNS = ("all", "none", "alternating", "tiles")


def seam_check(ctx, sizes, T, patterns=PATTERNS, bands=(mk.SUB, mk.PRESENT)):
    total = sum(sizes)
    queries = runs(sizes)
    qs = queries_of(ctx, queries)
    for name in patterns:
        refs = pattern_refs(name, total, T)
        idx = index_of(ctx, refs)
        for band in bands:
            want, st, sk = masked(ctx, qs, idx, refs, queries, band)
            if name == "all":
                assert st["kept"] == (total if band == mk.SUB else 0)
            if name == "none":
                assert st["kept"] == (0 if band == mk.SUB else total)


# ---- 1. the real reference's own sub ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,how", [("32", "built"), ("32", "imported"), ("64", "built"), ("64", "imported")])
def test_golden_pairs_equal_the_references_own_sub(ctx, tag, how):
    ref, qry, sub = golden(tag)
    wide, bits = (True, 36) if tag == "64" else (False, 24)
    idx = (index_of if how == "built" else imported_index)(ctx, ref, wide, bits)
    qs = queries_of(ctx, qry, wide)
    absent, st, _ = masked(ctx, qs, idx, ref, qry, mk.SUB)
    assert absent == [sorted(s.tolist()) for s in sub] and st["kept"] > 0   # the reference's own output, sketch by sketch
    present, st, _ = masked(ctx, qs, idx, ref, qry, mk.PRESENT)
    for q, a, b in zip(qry, absent, present):   # the complement
        assert sorted(a + b) == sorted(q.tolist()) and not set(a) & set(b)


# ---- 2. tiles, waves, sketch boundaries -------------------------------------------------------------------------------------------------
def test_totals_around_a_tile(ctx):
    T = tile_hashes(ctx)
    for total in (T - 1, T, T + 1, 2 * T + 1):
        seam_check(ctx, [total], T)
        seam_check(ctx, [total // 3, total - total // 3], T, patterns=("alternating",))


def test_a_sketch_boundary_at_every_offset_around_a_tile_and_a_wave_seam(ctx):
    T = tile_hashes(ctx)
    for b in list(range(T - 2, T + 3)) + list(range(62, 67)) + list(range(T + 62, T + 67)) + [T - 64, T + 64]:
        seam_check(ctx, [b, 2 * T + 5 - b], T, patterns=("alternating", "tiles"))
    seam_check(ctx, [T - 2, 1, 1, 1, 1, 62, 1, 1, 1], T, patterns=("all", "alternating"))   # a boundary at EVERY offset in [T - 2, T + 2] at once


def test_a_sketch_spanning_three_tiles(ctx):
    T = tile_hashes(ctx)
    seam_check(ctx, [T // 2, 2 * T + 10, 7], T)
    seam_check(ctx, [T - 1, T + 2, 1], T)        # its first and last tile hold one hash of it each


# ---- 3. empty sketches --------------------------------------------------------------------------------------------------------------------
def test_runs_of_empty_sketches(ctx):
    T = tile_hashes(ctx)
    seam_check(ctx, [0, 0, 0, 5, 0, 0, T - 5, 0, 0, 0, 70, 0, 0], T)          # at the start, in the middle, exactly on a tile boundary, at the end
    seam_check(ctx, [0, T, 0, 0, T, 0], T, patterns=("alternating", "tiles"))   # the LAST offsets lie on the boundary behind the last tile
    seam_check(ctx, [0, 0, 0], T, patterns=("all",))                              # nothing but empty sketches: no tile at all
    queries = [np.zeros(0, dtype=np.uint32)] * 3
    want, st, sk = masked(ctx, queries_of(ctx, queries), index_of(ctx, [np.array([5], dtype=np.uint32)]), [[5]], queries, mk.SUB)
    assert st["tiles"] == 0 and st["scan_blocks"] == 0 and sk.download()[1].tolist() == [0, 0, 0, 0]


# ---- 4. keep patterns ---------------------------------------------------------------------------------------------------------------------
def test_keep_patterns_over_several_tiles(ctx):
    T = tile_hashes(ctx)
    seam_check(ctx, [3 * T + 17, 0, 2 * T - 17, 40], T)   # all, none, alternating, and tiles that keep nothing between tiles that keep everything


# ---- 5. the scan at its seam --------------------------------------------------------------------------------------------------------------
def test_more_tiles_than_one_scan_block_takes(ctx):
    T = tile_hashes(ctx)
    S = scan_tiles(T)
    assert S * T * 4 <= 8 << 20   # a few MB of hashes
    total = S * T + 3 * T + 11
    every = np.arange(total, dtype=np.uint32)
    # a sketch boundary one before, on and one behind the seam of the scan blocks; tiles with everything, nothing and a mixture on either side
    sizes = [S * T // 2 + 3, 0, S * T // 2 - 4, 1, 1, 3 * T + 10]
    queries = runs(sizes)
    qs = queries_of(ctx, queries)
    for refs, bands in (([every[(every // 1000) % 3 == 0]], (mk.SUB, mk.PRESENT)), ([every[every >= S * T - 5]], (mk.SUB,))):
        idx = index_of(ctx, refs)
        for band in bands:
            want, st, sk = masked(ctx, qs, idx, refs, queries, band)
            assert st["scan_blocks"] >= 2 and st["tiles"] == S + 4 and 0 < st["kept"] < total


# ---- 6. the look-up at its edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_lookup_edges(ctx, wide):
    bits = 36 if wide else 24
    dtype = np.uint64 if wide else np.uint32
    top = (1 << 64) - 1 if wide else (1 << 32) - 1
    # indexed hashes on either side of every power of two: whatever the shift of the prefix directory, some are the first and some the
    # last hash of a bucket, and most buckets are empty
    indexed = sorted(set(x for s in range(8, bits) for x in ((1 << s) - 1, 1 << s, (1 << s) + 1)) | {200, (1 << bits) - 1})
    refs = [np.array(indexed, dtype=dtype), np.array(indexed[::2], dtype=dtype)]
    probe = set()
    for x in indexed:
        probe |= {x - 1, x, x + 1}
    # below the smallest and above the largest indexed hash, in empty buckets, at and beyond 2^hash_bits
    probe |= {0, 1, 199, 201, (1 << bits) - 2, 1 << bits, (1 << bits) + 1, (1 << bits) + 200, top - 1, top, 5 << (bits - 4), (5 << (bits - 4)) + 1}
    probe = sorted(p for p in probe if 0 <= p <= top)
    queries = [np.array(probe, dtype=dtype), np.array(probe[::3], dtype=dtype), np.array([1 << bits, top], dtype=dtype)]
    qs = queries_of(ctx, queries, wide)
    for make in (index_of, imported_index):
        if make is imported_index and not wide:
            continue   # (an import of 32-bit hashes uploads the dense 2^24 array: the golden case covers it)
        idx = make(ctx, refs, wide, bits)
        for band in (mk.SUB, mk.PRESENT, (1, 1), (2, 2)):
            want, st, _ = masked(ctx, qs, idx, refs, queries, band)
        assert want[2] == [] and st["matched"] == len(indexed) + len([p for p in probe[::3] if p in set(indexed)])
    # U = 1; an index of empty sketches; an index without genomes
    one = [np.array([77], dtype=dtype)]
    for refs1 in (one, [np.zeros(0, dtype=dtype)] * 2):
        idx = index_of(ctx, refs1, wide, bits)
        assert idx.distinct == (1 if refs1 is one else 0)
        q1 = [np.array([76, 77, 78], dtype=dtype), np.zeros(0, dtype=dtype)]
        for band in (mk.SUB, mk.PRESENT):
            masked(ctx, queries_of(ctx, q1, wide), idx, refs1, q1, band)
    none = device_index(ctx, np.zeros(0, dtype=dtype), np.zeros(1, dtype=np.uint64), bits, wide)
    assert none.genomes == 0
    want, st, _ = masked(ctx, qs, none, [], queries, mk.SUB)
    assert st["kept"] == st["hashes"] and st["matched"] == 0
    want, st, _ = masked(ctx, qs, none, [], queries, mk.PRESENT)
    assert st["kept"] == 0 and st["emptied"] == 3


# ---- 7. the band at its edges -------------------------------------------------------------------------------------------------------------
def test_band_edges(ctx):
    lengths = {10: 1, 20: 2, 30: 3, 650: 65}
    refs = [np.array(sorted(h for h, n in lengths.items() if r < n), dtype=np.uint32) for r in range(65)]
    idx = index_of(ctx, refs)
    queries = [np.array([5, 10, 20, 30, 650, 700], dtype=np.uint32), np.array([650], dtype=np.uint32)]
    qs = queries_of(ctx, queries)
    bounds = sorted(set(b for n in lengths.values() for b in (n - 1, n, n + 1)) | {mk.MAX})
    seen = set()
    for a in bounds:
        for b in bounds:
            if a <= b:
                want, st, _ = masked(ctx, qs, idx, refs, queries, (a, b))
                seen.add(tuple(want[0]))
    assert masked(ctx, qs, idx, refs, queries, (65, 65))[0] == [[650], [650]] and masked(ctx, qs, idx, refs, queries, (64, 64))[0] == [[], []]
    assert masked(ctx, qs, idx, refs, queries, (3, 3))[0] == [[30], []] and masked(ctx, qs, idx, refs, queries, (66, mk.MAX))[0] == [[], []]
    assert len(seen) >= 12


# ---- 8. repeats, on either side -------------------------------------------------------------------------------------------------------------
def takes_as_sets(ctx, idx, sk):
    """whether rk_gather_rows takes the object's sketches as sets: it refuses queries that repeat a hash (is_set false)"""
    try:
        ctx.gather_rows(idx, sk)
        return True
    except capi.RkError as e:
        assert e.code == RK_ERR_UNSUPPORTED
        return False


def test_repeated_query_hashes_keep_their_multiplicity(ctx):
    refs = [np.array([9, 12], dtype=np.uint32), np.array([9], dtype=np.uint32)]
    idx = index_of(ctx, refs)
    queries = [np.array([5, 5, 9, 9, 9, 11], dtype=np.uint32), np.array([9, 12, 12], dtype=np.uint32), np.array([3], dtype=np.uint32)]
    qs = queries_of(ctx, queries)
    want, st, sk = masked(ctx, qs, idx, refs, queries, mk.SUB)
    assert want == [[5, 5, 11], [], [3]] and not takes_as_sets(ctx, idx, sk)
    want, st, sk = masked(ctx, qs, idx, refs, queries, mk.PRESENT)
    assert want == [[9, 9, 9], [9, 12, 12], []] and not takes_as_sets(ctx, idx, sk)
    want, st, sk = masked(ctx, qs, idx, refs, queries, (1, 1))
    assert want == [[], [12, 12], []] and not takes_as_sets(ctx, idx, sk)
    # every repeat is dropped: the result is a set again -- also where a sketch begins with the hash the one before it ends with
    queries = [np.array([5, 5, 9], dtype=np.uint32), np.array([9, 12], dtype=np.uint32), np.array([12, 12, 13], dtype=np.uint32)]
    refs = [np.array([5, 12], dtype=np.uint32)]
    idx = index_of(ctx, refs)
    want, st, sk = masked(ctx, queries_of(ctx, queries), idx, refs, queries, mk.SUB)
    assert want == [[9], [9], [13]] and takes_as_sets(ctx, idx, sk)
    want, st, sk = masked(ctx, queries_of(ctx, queries), idx, refs, queries, mk.PRESENT)
    assert want == [[5, 5], [12], [12, 12]] and not takes_as_sets(ctx, idx, sk)
    sets = [np.array([5, 9], dtype=np.uint32), np.array([9, 12], dtype=np.uint32)]
    want, st, sk = masked(ctx, queries_of(ctx, sets), idx, refs, sets, mk.SUB)
    assert want == [[9], [9]] and takes_as_sets(ctx, idx, sk)


def test_a_reference_that_repeats_a_hash_counts_it_twice(ctx):
    refs = [np.array([7, 7, 8], dtype=np.uint32), np.array([8, 9], dtype=np.uint32)]
    idx = index_of(ctx, refs)
    queries = [np.array([6, 7, 8, 9], dtype=np.uint32)]
    qs = queries_of(ctx, queries)
    assert masked(ctx, qs, idx, refs, queries, (2, 2))[0] == [[7, 8]]
    assert masked(ctx, qs, idx, refs, queries, (1, 1))[0] == [[9]]
    assert masked(ctx, qs, idx, refs, queries, mk.SUB)[0] == [[6]]


# ---- 9. 36-bit hashes and random collections, every band ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_random_collections_through_every_band(ctx, wide):
    bits, kmer = (36, 24) if wide else (24, 20)
    dtype = np.uint64 if wide else np.uint32
    names, h, off = synth.clade_sketches(300, 60, bits, kmer_size=kmer, strains_per_clade=10, seed=23 + wide, wide=wide)
    refs = mk.parts_of(h, off)
    rng = np.random.default_rng(5 + wide)
    T = tile_hashes(ctx)
    queries = []
    for k in range(60):
        members = rng.choice(len(refs), size=1 + k % 5, replace=False)
        foreign = rng.integers(0, 1 << bits, size=int(rng.integers(0, 40)), dtype=np.uint64)
        queries.append(np.unique(np.concatenate([refs[m].astype(np.uint64) for m in members] + [foreign])).astype(dtype))
    queries[7] = np.zeros(0, dtype=dtype)
    assert sum(len(q) for q in queries) > 2 * T
    qs = queries_of(ctx, queries, wide)
    for make in (index_of, imported_index) if wide else (index_of,):
        idx = make(ctx, refs, wide, bits)
        kept = set()
        for band in BANDS + [(0, 9), (10, mk.MAX), (10, 10)]:
            want, st, _ = masked(ctx, qs, idx, refs, queries, band)
            kept.add(st["kept"])
        assert len(kept) >= 6


# ---- 10. the result fed onward ----------------------------------------------------------------------------------------------------------------
def test_the_result_goes_into_the_index_build_and_the_self_join(ctx):
    ref, qry, sub = golden("32")
    sk = masked(ctx, queries_of(ctx, qry), index_of(ctx, ref), ref, qry, mk.SUB)[2]
    host_h, host_off = csr([np.array(k, dtype=np.uint32) for k in mk.from_counter(ref, [sorted(q.tolist()) for q in qry], *mk.SUB)])
    want = Oracle(host_h, host_off, 24).hits(0, 1.5)
    mine = ctx.dist_rows(ctx.index_build(sk, 24), None, 1, 0, KMER, 1.5)[0]
    assert len(mine) == len(want) > 0
    key = lambda r: np.lexsort((r["col"], r["row"]))   # noqa: E731
    for f in ("row", "col", "common", "size0", "size1"):
        assert np.array_equal(mine[f][key(mine)], want[f][key(want)]), f
    assert np.max(np.abs(mine["dist"][key(mine)] - want["dist"][key(want)])) <= 1e-12


@pytest.mark.parametrize("tag", ["32", "64"])
def test_the_result_goes_into_gather(ctx, tag):
    ref, qry, sub = golden(tag)
    wide, bits = (True, 36) if tag == "64" else (False, 24)
    host = ref[:len(ref) // 2]            # the queries lose what half of the references hold, and are covered by all of them
    sk = masked(ctx, queries_of(ctx, qry, wide), index_of(ctx, host, wide, bits), host, qry, mk.SUB)[2]
    subtracted = mk.from_counter(host, [sorted(q.tolist()) for q in qry], *mk.SUB)
    (off, picks, matched, n_cand, covered), st = gathered(ctx, index_of(ctx, ref, wide, bits), sk, ref, subtracted)
    assert len(picks) >= 1 and 0 < sum(matched) < sum(len(q) for q in subtracted)   # (the picks themselves: compared in gathered)


# ---- 11. the host leg ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_the_host_leg_gives_the_same_arrays(ctx, wide, monkeypatch):
    ref, qry, sub = golden("64" if wide else "32")
    bits = 36 if wide else 24
    dtype = np.uint64 if wide else np.uint32
    queries = qry + [np.array([5, 5, 9], dtype=dtype), np.array([1 << bits, (1 << bits) + 1], dtype=dtype)]
    qs = queries_of(ctx, queries, wide)
    idx = index_of(ctx, ref, wide, bits)
    none = device_index(ctx, np.zeros(0, dtype=dtype), np.zeros(1, dtype=np.uint64), bits, wide)
    for band in BANDS:
        device = masked(ctx, qs, idx, ref, queries, band)[2].download()
        monkeypatch.setenv("RK_MASK_DEVICE", "0")
        want, st, sk = masked(ctx, qs, idx, ref, queries, band, path=2)
        masked(ctx, qs, none, [], queries, band, path=2)
        monkeypatch.delenv("RK_MASK_DEVICE")
        host = sk.download()
        assert device[0].tobytes() == host[0].tobytes() and device[1].tobytes() == host[1].tobytes()


# ---- 12. what is refused --------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, qs, idx, rule=(0, 0), skip=None):
    L = capi.lib()
    L.rk_sketches_mask.argtypes = MASK_ARGTYPES
    out = C.c_void_p(0x1234)
    r = capi.MaskRule(*rule) if rule is not None else None
    st = capi.MaskStats()
    args = [ctx._h, qs._h if qs is not None else None, idx._h if idx is not None else None, C.byref(r) if r is not None else None, C.byref(out), C.byref(st)]
    if skip is not None:
        args[skip] = None
    rc = L.rk_sketches_mask(*args)
    return rc, out.value == 0x1234 and st.path == 0 and st.hashes == 0


def test_arguments_that_are_refused(ctx):
    ref, qry, sub = golden("32")
    wref, wqry, wsub = golden("64")
    idx, qs = index_of(ctx, ref), queries_of(ctx, qry)
    last = lambda: capi.lib().rk_last_error(ctx._h)   # noqa: E731
    assert raw_call(ctx, qs, idx, (2, 1)) == (RK_ERR_ARG, True) and b"min_refs" in last()
    assert raw_call(ctx, qs, idx, None) == (RK_ERR_ARG, True)
    for skip in (1, 2, 4):   # queries, idx, out
        assert raw_call(ctx, qs, idx, skip=skip) == (RK_ERR_ARG, True), skip
    assert raw_call(ctx, queries_of(ctx, wqry, True), idx) == (RK_ERR_ARG, True) and b"widths" in last()
    assert raw_call(ctx, qs, index_of(ctx, wref, True, 36)) == (RK_ERR_ARG, True) and b"widths" in last()
    with pytest.raises(capi.RkError) as e:
        ctx.sketches_mask(qs, idx, 3, 2)
    assert e.value.code == RK_ERR_ARG
    # no query sketch: RK_OK, no object, nothing ran -- and the stats are optional
    none_q = ctx.sketches_from_host(np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64))
    sk, st = ctx.sketches_mask(none_q, idx, 0, 0)
    assert sk is None and st["path"] == 0 and st["hashes"] == st["tiles"] == st["tile_hashes"] == 0
    L = capi.lib()
    out = C.c_void_p(0x1234)
    r = capi.MaskRule(0, 0)
    assert L.rk_sketches_mask(ctx._h, qs._h, idx._h, C.byref(r), C.byref(out), None) == 0 and out.value not in (None, 0x1234)
    L.rk_sketches_free(out)


def test_indexes_without_all_posting_lists_are_refused(ctx):
    import torch
    S = 2
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    sk = ctx.sketches_from_host(h, off)
    qs = queries_of(ctx, mk.parts_of(h, off)[:3])
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    assert raw_call(ctx, qs, parts[0]) == (RK_ERR_ARG, True)   # one hash range of a sharded build
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
    assert raw_call(ctx, qs, j) == (RK_ERR_ARG, True)   # the join-only index: tile records of its rows, no lists
    assert b"posting lists" in capi.lib().rk_last_error(ctx._h)
    del j, parts, sk


# ---- 13. the tool -----------------------------------------------------------------------------------------------------------------------------------
def run_tool(cwd, args):
    return subprocess.run([TOOL] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def golden_files(tag, tmp_path):
    d, s = ("dist64", "64") if tag == "64" else ("dist", "")
    shutil.copy(os.path.join(GOLDEN, d, "ref%s.sketch" % s), tmp_path / "ref.sketch")
    shutil.copy(os.path.join(GOLDEN, d, "qry%s.sketch" % s), tmp_path / "qry.sketch")
    return ok.read_sketches64 if tag == "64" else ok.read_sketches32


@pytest.mark.parametrize("tag", ["32", "64"])
def test_tool_mask_writes_the_references_sub(ctx, tag, tmp_path):
    read = golden_files(tag, tmp_path)
    w_info, w_names, w_h, w_off = read(os.path.join(GOLDEN, "f4", "sub%s.sketch" % tag))
    want = [sorted(p.tolist()) for p in mk.parts_of(w_h, w_off)]
    for round_, extra in enumerate(([], ["--keep", "absent"])):   # first without the .dict / .index pair (it is written), then with it
        assert (tmp_path / "ref.sketch.dict").exists() == (tmp_path / "ref.sketch.index").exists() == (round_ == 1)
        p = run_tool(tmp_path, ["mask", "-r", "ref.sketch", "-q", "qry.sketch", "-o", "out%d.sketch" % round_] + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        info, names, h, off = read(str(tmp_path / ("out%d.sketch" % round_)))
        assert bytes(info) == bytes(w_info) and names == w_names and np.array_equal(off, w_off)
        assert [p.tolist() for p in mk.parts_of(h, off)] == want     # the reference's hashes, ascending within a sketch
    assert (tmp_path / "out0.sketch").read_bytes() == (tmp_path / "out1.sketch").read_bytes()


def test_tool_mask_bands_and_what_dies(ctx, tmp_path):
    ref, qry, sub = golden("32")
    read = golden_files("32", tmp_path)
    sorted_q = [sorted(q.tolist()) for q in qry]
    for args, band in ((["--keep", "present"], mk.PRESENT), (["--min-refs", "2"], (2, mk.MAX)), (["--max-refs", "1"], (0, 1)),
                       (["--min-refs", "8", "--max-refs", "9"], (8, 9)), (["--min-refs", "1", "--max-refs", "1"], (1, 1))):
        p = run_tool(tmp_path, ["mask", "-r", "ref.sketch", "-q", "qry.sketch", "-o", "out.sketch"] + args)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        info, names, h, off = read(str(tmp_path / "out.sketch"))
        want = mk.from_counter(ref, sorted_q, *band)
        assert [p.tolist() for p in mk.parts_of(h, off)] == want and sum(len(k) for k in want) > 0, args
    base = ["mask", "-r", "ref.sketch", "-q", "qry.sketch", "-o", "x.sketch"]
    for args, text in ((["mask", "-r", "ref.sketch", "-o", "x.sketch"], b"needs -r, -q and -o"), (["mask", "-r", "ref.sketch", "-q", "qry.sketch"], b"needs -r, -q and -o"),
                       (base + ["--gpus", "2"], b"one GPU"), (base + ["--keep", "some"], b"--keep must be absent or present"),
                       (base + ["--keep", "present", "--min-refs", "1"], b"exclude each other"), (base + ["--min-refs", "3", "--max-refs", "2"], b"must not exceed"),
                       (base + ["--min-refs", "-1"], b"needs an integer"), (base + ["--max-refs", "4294967296"], b"needs an integer")):
        p = run_tool(tmp_path, args)
        assert p.returncode != 0 and text in p.stderr and not (tmp_path / "x.sketch").exists(), args
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"mask    -r" in p.stderr and b" info mask\n" in p.stderr and b"--sub host.sketch" in p.stderr


def test_tool_gather_sub_equals_gather_over_what_sub_wrote(ctx, tmp_path):
    golden_files("32", tmp_path)
    shutil.copy(os.path.join(GOLDEN, "f4", "merge32.sketch"), tmp_path / "all.sketch")   # the queries and the references in one collection
    p = run_tool(tmp_path, ["sub", "--rs", "ref.sketch", "--qs", "qry.sketch", "-o", "subbed.sketch"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    p = run_tool(tmp_path, ["gather", "-r", "all.sketch", "-q", "subbed.sketch", "-o", "a.txt", "--summary", "sa.txt"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    p = run_tool(tmp_path, ["gather", "-r", "all.sketch", "-q", "qry.sketch", "--sub", "ref.sketch", "-o", "b.txt", "--summary", "sb.txt"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes() and len((tmp_path / "a.txt").read_text().splitlines()) >= 12
    assert (tmp_path / "sa.txt").read_bytes() == (tmp_path / "sb.txt").read_bytes()
    p = run_tool(tmp_path, ["gather", "-r", "all.sketch", "-q", "qry.sketch", "-o", "c.txt"])   # without the flag nothing changes
    assert p.returncode == 0 and (tmp_path / "c.txt").read_bytes() != (tmp_path / "a.txt").read_bytes()
    p = run_tool(tmp_path, ["gather", "-r", "all.sketch", "-q", "qry.sketch", "--sub", "ref.txt", "-o", "d.txt"])
    assert p.returncode != 0 and b"--sub needs a sketch file" in p.stderr and not (tmp_path / "d.txt").exists()
