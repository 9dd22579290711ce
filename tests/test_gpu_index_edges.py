"""The index build at its switches (rk_index.hip, rk_index_plan.h, rk_index_fast.inc, rk_index_tiles.inc): key widths, bucket and
sub-bucket capacity, the chunk geometry of the partition walk, knobs, attempts that carry state, the internal order.

The build degrades silently -- an attempt is repeated, tile records become slice records, a raised flag sends the collection to the
device-wide sort, and the index is right by construction --, so an index that equals the oracle's proves nothing about the kernels
at an edge.  Every leg therefore first asserts WHICH build ran: rk_index_build_plan against the plan words the case is about
(evaluated by hand in tests/_index_cases.py, whose generators also assert the exact bucket sizes and chunk boundaries on the CPU),
then rk_index_build_report (attempts, retries, fallback, general path, flags, buckets left to k_bucket_heavy), and only then the
index: .dict / .index content, the internal order against its numpy reference, the count of slice or tile records, the hits of a
tight and a loose self join.  Everything compared is an integer or a double computed on the host: no tolerance."""
import numpy as np
import pytest

import _index_cases as ic
from _order_ref import order_ref
from oracle import oracle as ok
from rabbitkssd_amd import capi

pytestmark = pytest.mark.gpu
KMER = 20
THRESHOLDS = (0.05, 1.0)
# what a context or a build reads of the environment: a leg runs under ITS settings alone
KNOBS = ("RK_INDEX_PASS_BITS", "RK_INDEX_BUCKET_TARGET", "RK_INDEX_ONE_STREAM", "RK_INDEX_STREAM2_PRIO", "RK_INDEX_TABLE_X", "RK_INDEX_XCD",
         "RK_INDEX_KEYS_CAP_PCT", "RK_INDEX_PART2", "RK_INDEX_FILTER", "RK_INDEX_EMIT_T", "RK_INDEX_DEBUG", "RK_INDEX_FAST", "RK_INDEX_RELABEL",
         "RK_INDEX_NO_SELF", "RK_INDEX_TILES", "RK_INDEX_NO_HEAVY", "RK_TILE_REC_CAP", "RK_DIST_TILES", "RK_DIST_TILES_MIN_GENOMES")

_REFS = {}


def assert_hits_equal(mine, want, what):
    assert len(mine) == len(want), "%s: %d hits against %d" % (what, len(mine), len(want))
    for f in ("row", "col", "common", "size0", "size1"):
        assert np.array_equal(mine[f], want[f]), "%s: %s" % (what, f)
    assert np.array_equal(mine["jorc"], want["jorc"]), what            # one IEEE division
    assert np.array_equal(mine["dist"], want["dist"]), what            # rk_dist_rows recomputes it with the host's libm


def reference(h, off, bits):
    """the oracle's index and self-join hits of a collection, computed once (the generators hand out one copy of each collection)"""
    ref = _REFS.get(id(h))
    if ref is None:
        sizes = np.diff(off.astype(np.int64)).astype(np.uint32)
        if h.dtype == np.uint64 or bits > 28:     # the sparse .dict / .index of 64-bit hashes; a 32-bit space has no dense array either
            h64 = h.astype(np.uint64)
            uhash, ucount, postings = ok.index_build64(h64, off)
            hits = {D: ok.index_dist64(uhash, ucount, postings, sizes, h64, off, 1, 0, KMER, D, threads=8)[0] for D in THRESHOLDS}
            ref = {"keep": h, "postings": postings, "hashes": uhash, "counts": ucount, "lists": ucount, "hits": hits}
        else:
            postings, counts = ok.index_build32(h, off, bits)
            hits = {D: ok.index_dist32(counts, bits, postings, sizes, h, off, 1, 0, KMER, D, threads=8)[0] for D in THRESHOLDS}
            ref = {"keep": h, "postings": postings, "hashes": None, "counts": counts, "lists": counts[counts > 0], "hits": hits}
        ref["order"] = order_ref(h, off)
        _REFS[id(h)] = ref
    return ref


def check_leg(monkeypatch, case, leg):
    h, off, bits, env, expect = ic.make(case, leg)
    ref = reference(h, off, bits)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = capi.Context(0)
    try:
        sk = c.sketches_from_host64(h, off) if h.dtype == np.uint64 else c.sketches_from_host(h, off)
        # 1. the build this leg is about is the one that will run
        plan = c.index_build_plan(sk, bits)
        assert {k: plan[k] for k in expect["plan"]} == expect["plan"], "plan: %r" % (plan,)
        idx = c.index_build(sk, bits)
        # 2. ... and the one that did
        report = idx.build_report
        assert {k: report[k] for k in expect["report"]} == expect["report"], "report: %r" % (report,)
        assert idx.built_fast == (report["general"] == 0) and idx.products == expect["products"]
        # 3. the .dict / .index content
        H, lists = len(h), ref["lists"]
        if ref["hashes"] is None:
            postings, counts = idx.export()
            assert np.array_equal(postings, ref["postings"]) and np.array_equal(counts, ref["counts"])
        else:
            postings, hashes, counts = idx.export64() if h.dtype == np.uint64 else idx.export_lists()
            assert np.array_equal(postings, ref["postings"]) and np.array_equal(hashes.astype(np.uint64), ref["hashes"])
            assert np.array_equal(counts, ref["counts"])
        assert idx.total == H and idx.genomes == len(off) - 1 and idx.distinct == len(lists)
        assert idx.sum_sq == int((lists.astype(np.int64) ** 2).sum())
        # 4. the internal order
        order = idx.order
        assert np.array_equal(order, np.arange(len(order)) if env.get("RK_INDEX_RELABEL") == "0" else ref["order"])
        # 5. as many slice or tile records as the lists and that order ask for
        stats = idx.self_stats
        if expect["products"] & 1:
            assert stats[0] == H - len(lists)
        else:
            assert stats[3] == ic.tile_records_ref(ref["postings"], lists, order)
        if "tile_records" in expect:
            assert stats[3] == expect["tile_records"]
        # 6. the self join, tight and loose
        for D in THRESHOLDS:
            assert_hits_equal(c.dist_rows(idx, None, 1, 0, KMER, D)[0], ref["hits"][D], "D=%g" % D)
        del idx, sk
    finally:
        c.close()


@pytest.mark.parametrize("case,leg", ic.all_legs(), ids=["%s-%s" % cl for cl in ic.all_legs()])
def test_index_build_edge(monkeypatch, case, leg):
    check_leg(monkeypatch, case, leg)


def test_plan_refuses_what_the_build_refuses_and_the_report_of_other_indexes_is_zero(monkeypatch):
    import torch
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    h, off, bits, env, expect = ic.make("part2_threshold", "b6")
    ref = reference(h, off, bits)
    c = capi.Context(0)
    try:
        sk = c.sketches_from_host(h, off)
        with pytest.raises(capi.RkError, match="does not match"):       # plan_build's own refusal, word for word the build's
            c.index_build_plan(sk, 36)
        with pytest.raises(capi.RkError, match="does not match"):
            c.index_build(sk, 36)
        with pytest.raises(capi.RkError, match="shards"):
            c.index_build_plan(sk, bits, 3, 3)
        assert c.index_build_plan(sk, bits, 1, 4)["range_bits"] == 2 and c.index_build_plan(sk, bits, 1, 4)["tiles_mode"] == 1
        built = c.index_build(sk, bits)
        assert built.build_report["attempts"] == 1
        zeros = dict.fromkeys(capi.REPORT_WORDS, 0)
        imported = c.index_import(ref["postings"], ref["counts"], bits, np.diff(off.astype(np.int64)))
        assert imported.build_report == zeros
        blob = torch.empty(built.blob_bytes, dtype=torch.uint8, device="cuda")
        built.pack_dev(blob.data_ptr(), built.blob_bytes)
        torch.cuda.synchronize()
        assert c.index_unpack_dev(blob.data_ptr(), built.blob_bytes).build_report == zeros
    finally:
        c.close()
