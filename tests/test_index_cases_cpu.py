"""CPU-only checks of what the index build's edge tests (test_gpu_index_edges.py) stand on: every case generator of _index_cases runs
and meets the preconditions it asserts, and the two references -- the internal order (_order_ref) and the count of tile records --
give the obvious answer on collections small enough to work out by hand."""
import numpy as np
import pytest

import _index_cases as ic
from _order_ref import fold32, order_ref, parents_ref
from rabbitkssd_amd import capi


def csr(parts, dtype=np.uint32):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return np.concatenate([np.asarray(p, dtype=dtype) for p in parts]), off


@pytest.mark.parametrize("case,leg", ic.all_legs())
def test_case_generators_meet_their_preconditions(case, leg):
    h, off, bits, env, expect = ic.make(case, leg)
    n = len(off) - 1
    assert off[0] == 0 and off[-1] == len(h) and n <= 33000 and len(h) <= 1_100_000
    assert h.dtype == (np.uint64 if bits > 32 else np.uint32) and (bits == 64 or int(h.max()) < (1 << bits))
    for g in np.flatnonzero(np.diff(off.astype(np.int64)) > 1)[:: max(1, n // 50)]:       # (set sketches: a sample; csr() checked them all)
        s = h[int(off[g]): int(off[g + 1])]
        assert np.all(s[1:] > s[:-1])
    assert set(expect["plan"]) <= set(capi.PLAN_WORDS) and set(expect["report"]) <= set(capi.REPORT_WORDS)
    assert all(k.startswith("RK_") and isinstance(v, str) for k, v in env.items())
    assert expect["products"] in (1, 6)


def test_every_case_of_the_table_is_there():
    assert list(ic.CASES) == ["low_bits_0", "low_bits_31_32", "narrow_32_33", "key_equals_padding", "part2_threshold", "coarse_variants",
                              "bucket_capacity", "crowded_sub_bucket", "chunk_geometry", "attempts", "order"]
    assert len(ic.all_legs()) == len(set(ic.all_legs())) == 80


def test_order_one_shared_hash_does_not_attach_two_do():
    h, off = csr([[10, 20, 30], [10, 40, 50], [10, 20, 60], [70, 80, 90]])
    assert parents_ref(h, off).tolist() == [0, 1, 0, 3]            # genome 1 shares one hash with 0, genome 2 two
    assert order_ref(h, off).tolist() == [0, 2, 1, 3]


def test_order_a_chain_ends_at_its_first_genome():
    a, b, c = [1, 2, 3, 4], [3, 4, 5, 6], [5, 6, 7, 8]               # c shares nothing with a
    h, off = csr([a, [100, 200], b, [300], c])
    assert parents_ref(h, off).tolist() == [0, 1, 0, 3, 2]
    assert order_ref(h, off).tolist() == [0, 2, 4, 1, 3]             # by (root, caller's index): 0, 2, 4 have root 0


def test_order_attaches_to_the_smaller_of_two_candidates():
    h, off = csr([[1, 2, 50], [3, 4, 60], [70, 80], [1, 2, 3, 4]])
    assert parents_ref(h, off).tolist() == [0, 1, 2, 0]
    h, off = csr([[3, 4, 60], [1, 2, 50], [70, 80], [1, 2, 3, 4]])   # the same two candidates listed the other way round
    assert parents_ref(h, off).tolist() == [0, 1, 2, 0]
    assert order_ref(h, off).tolist() == [0, 3, 1, 2]


def test_order_sketches_of_0_1_and_15_hashes_and_the_limit_of_16():
    big = list(range(1000, 1015))                                    # 15 hashes
    h, off = csr([[], [5], big, [5], [], big[:2] + [2000]])
    assert parents_ref(h, off).tolist() == [0, 1, 2, 3, 4, 2]        # one shared hash (genomes 1 and 3) is one vote; empty sketches stay
    assert order_ref(h, off).tolist() == [0, 1, 2, 5, 3, 4]
    # only the first 16 hashes count: genomes that share their 17th and 18th do not attach, genomes that share the 15th and 16th do
    a = list(range(100, 116)) + [900, 901]
    b = list(range(200, 216)) + [900, 901]
    h, off = csr([a, b])
    assert parents_ref(h, off).tolist() == [0, 1]
    c = [114, 115] + list(range(300, 314))
    h, off = csr([a, b, c])
    assert parents_ref(h, off).tolist() == [0, 1, 0]


def test_order_two_64bit_hashes_that_fold_to_the_same_32_bits():
    x, y = np.uint64((3 << 32) | 0x10), np.uint64((1 << 32) | 0x12)     # 0x10 ^ 3 == 0x12 ^ 1 == 0x13
    assert x != y and fold32(np.array([x, y])).tolist() == [0x13, 0x13]
    p, q = np.uint64((2 << 32) | 0x40), np.uint64(0x42)                # both fold to 0x42
    h, off = csr([[q, y, 1 << 35], [x, p, 1 << 34]], np.uint64)
    assert len(np.intersect1d(h[:3], h[3:])) == 0                      # no hash in common, two folds in common
    assert parents_ref(h, off).tolist() == [0, 0]
    h, off = csr([[q, 7, 1 << 35], [x, p, 1 << 34]], np.uint64)        # one fold in common
    assert parents_ref(h, off).tolist() == [0, 1]
    # inside ONE sketch two hashes with the same fold are two votes for that fold's owner
    z = np.uint64((2 << 32) | 0x11)                                    # 0x11 ^ 2 == 0x13 as well
    h, off = csr([[9, y], [z, x]], np.uint64)
    assert fold32(h).tolist() == [9, 0x13, 0x13, 0x13] and parents_ref(h, off).tolist() == [0, 0]


def test_tile_records_of_three_lists_counted_by_hand():
    order = np.arange(100)
    # list A = {0, 1, 40}: runs {0, 1} and {40}: one pair of runs + one run of two members = 2 records
    # list B = {5}: one run of one member = 0 records
    # list C = {2, 33, 34, 70, 99}: runs {2}, {33, 34}, {70}, {99}: six pairs + one run of two = 7 records
    postings = np.array([0, 1, 40, 5, 2, 33, 34, 70, 99])
    assert ic.tile_records_ref(postings[:3], [3], order) == 2
    assert ic.tile_records_ref(postings[3:4], [1], order) == 0
    assert ic.tile_records_ref(postings[4:], [5], order) == 7
    assert ic.tile_records_ref(postings, [3, 0, 1, 0, 0, 5], order) == 9            # (a dense count array: zeros are skipped)
    # another internal order moves the runs: genome 40 becomes internal id 2, genome 2 internal id 40
    swapped = order.copy()
    swapped[[2, 40]] = [40, 2]
    assert ic.tile_records_ref(postings[:3], [3], swapped) == 1                      # {0, 1, 40} is one run of three
    assert ic.tile_records_ref(postings[4:], [5], swapped) == 3 + 1                  # runs {33, 34, 2 -> 40}, {70}, {99}


def test_region_records_add_up_to_the_tile_records():
    # per region the same count as tile_records_ref over all lists; a bucket's records go to region bucket % 64
    h, off, bits, env, expect = ic.make("bucket_capacity", "tiles-4097")
    from oracle import oracle as ok
    postings, counts = ok.index_build32(h, off, bits)
    order = order_ref(h, off)
    asked = ic.region_records(h, off, bits, 5, order)
    assert asked.sum() == ic.tile_records_ref(postings, counts, order) and asked[32:].sum() == 0
    h, off = csr([[0x10, 0x2000000], [0x10, 0x2000000], [0x10] * 0 + [0x2000000]] + [[]] * 30 + [[0x10]])
    # list 0x10 (bucket 0): genomes 0, 1, 33: runs {0, 1}, {33}: 2 records; list 0x2000000 (bucket 16 of 32): genomes 0, 1, 2: 1 record
    asked = ic.region_records(h, off, 26, 5, np.arange(34))
    assert asked[0] == 2 and asked[16] == 1 and asked.sum() == 3
