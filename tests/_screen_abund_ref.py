"""The rule of rk_screen_abund_rows / rk_screen_abund_lists in plain Python, twice and independently: from per-query dicts hash -> count
(the definition of include/rabbitkssd.h: containments as fractions.Fraction, every candidate scanned per hash, statistics.median_low) and
from posting lists plus the counts of the hashes that hit them (the row's candidates ranked once, the median as the element of rank
(n - 1) // 2 of the sorted values).  Integers and exact fractions only.  tests/test_screen_abund_cpu.py checks the two against each other and
against the facts that follow from the rule; everything else is checked against them.  No test lives here.

    refs      a list of iterables of hashes, taken as sets
    queries   a list of dicts hash -> count (count >= 1)
    result    per query (recs, abund, matched, n_cand, claimed, occ): recs as tests/_screen_ref.py has them, (query, ref, common, won);
              abund parallel to recs, the tuple ABUND_FIELDS; occ = the sums of the counts over the whole sketch, the matched and the
              claimed hashes"""
import functools
import itertools
import statistics
import struct
from fractions import Fraction

import numpy as np

import _screen_ref as sr

ABUND_FIELDS = ("occ_common", "occ_won", "med_common", "med_won")


def summary(shared, claimed):
    """the abundance record of a reference from the counts of the hashes it shares and of those it claims"""
    return (sum(shared), sum(claimed), statistics.median_low(shared), statistics.median_low(claimed) if claimed else 0)


def from_dicts(refs, queries, min_common=1, min_won=0, sizes=None):
    """the definition: per matched hash the best of its holders that are candidates -- the larger containment (an exact fraction), then
    the larger size, then the smaller index -- takes the hash and its count"""
    assert min_common >= 1
    R = [set(int(h) for h in r) for r in refs]
    size = sr.sizes_of(refs, sizes)
    indexed = set().union(*R) if R else set()
    out = []
    for q, m in enumerate(queries):
        S = set(int(h) for h in m)
        assert all(c >= 1 for c in m.values())
        common = [len(S & r) for r in R]
        cands = [r for r in range(len(R)) if common[r] >= min_common]
        key = {r: (Fraction(common[r], size[r]), size[r], -r) for r in cands}
        claimed_by = {r: [] for r in cands}
        occ_claimed = 0
        for h in sorted(S & indexed):
            holders = [r for r in cands if h in R[r]]
            if holders:
                claimed_by[max(holders, key=key.__getitem__)].append(m[h])
                occ_claimed += m[h]
        recs, abund = [], []
        for r in cands:
            if len(claimed_by[r]) >= min_won:
                recs.append((q, r, common[r], len(claimed_by[r])))
                abund.append(summary([m[h] for h in S & R[r]], claimed_by[r]))
        out.append((recs, abund, len(S & indexed), len(cands), sum(len(v) for v in claimed_by.values()),
                    (sum(m.values()), sum(m[h] for h in S & indexed), occ_claimed)))
    return out


def lower_median(values):
    return sorted(values)[(len(values) - 1) // 2]


def from_lists(lists, n_ref, queries, sizes, min_common=1, min_won=0):
    """from posting lists ({hash: the references that hold it}) and the counts of the hashes that hit them: the counters per reference, the
    row's candidates ranked once with the integer comparator, a list and its count go to its member of the smallest rank"""
    assert min_common >= 1
    out = []
    for q, m in enumerate(queries):
        live = [(lists[h], m[h]) for h in sorted(m) if h in lists]   # (list, q_count)
        common = [0] * n_ref
        for l, _ in live:
            for r in l:
                common[r] += 1
        cands = [r for r in range(n_ref) if common[r] >= min_common]
        order = sorted(((common[r], sizes[r], r) for r in cands), key=functools.cmp_to_key(sr.better))
        rank = {k[2]: i for i, k in enumerate(order)}
        shared, claimed_by = {r: [] for r in cands}, {r: [] for r in cands}
        occ_claimed = 0
        for l, c in live:
            ranks = [rank[r] for r in l if r in rank]
            for r in l:
                if r in rank:
                    shared[r].append(c)
            if ranks:
                claimed_by[order[min(ranks)][2]].append(c)
                occ_claimed += c
        recs = [(q, r, common[r], len(claimed_by[r])) for r in cands if len(claimed_by[r]) >= min_won]
        abund = [(sum(shared[r]), sum(claimed_by[r]), lower_median(shared[r]), lower_median(claimed_by[r]) if claimed_by[r] else 0) for _, r, _, _ in recs]
        out.append((recs, abund, len(live), len(cands), sum(len(v) for v in claimed_by.values()), (sum(m.values()), sum(c for _, c in live), occ_claimed)))
    return out


def fast(refs, queries, min_common=1, min_won=0, sizes=None):
    return from_lists(sr.posting_lists(refs), len(refs), queries, sr.sizes_of(refs, sizes), min_common, min_won)


def facts(refs, queries, result, min_common=1, min_won=0, sizes=None):
    """the facts that follow from the rule; raises AssertionError"""
    plain = sr.fast(refs, [list(m) for m in queries], min_common, min_won, sizes)
    every = result if min_won == 0 else fast(refs, queries, min_common, 0, sizes)
    for (recs, abund, matched, n_cand, claimed, occ), (p_recs, p_matched, p_cand, p_claimed), (_, all_abund, _, _, _, _) in zip(result, plain, every):
        assert (recs, matched, n_cand, claimed) == (p_recs, p_matched, p_cand, p_claimed)   # the records are the screen's
        assert len(abund) == len(recs)
        for (_, _, common, won), (occ_common, occ_won, med_common, med_won) in zip(recs, abund):
            assert occ_won <= occ_common and common <= occ_common and won <= occ_won
            assert (med_won == 0) == (won == 0) and med_common >= 1
        assert sum(a[1] for a in all_abund) == occ[2] <= occ[1] <= occ[0]                 # what the records claim is what the row claims
        if min_common == 1:
            assert occ[1] == occ[2]
    ones = [{h: 1 for h in m} for m in queries]
    if ones != queries:   # with all counts 1 every sum is the cardinality and every non-empty median 1
        for (recs, abund, matched, n_cand, claimed, occ), m in zip(fast(refs, ones, min_common, min_won, sizes), ones):
            assert occ == (len(m), matched, claimed)
            assert abund == [(common, won, 1, 1 if won else 0) for _, _, common, won in recs]


def exported(refs, queries):
    """(postings, counts, q_off, q_lists, q_counts, query_occ) as rk_screen_abund_lists takes them: the lists in ascending hash order"""
    postings, counts, q_off, q_lists = sr.exported(refs, [list(m) for m in queries])
    hashes = sorted(sr.posting_lists(refs))
    q_counts = [queries[q][hashes[u]] for q in range(len(queries)) for u in q_lists[q_off[q]:q_off[q + 1]]]
    return postings, counts, q_off, q_lists, q_counts, [sum(m.values()) for m in queries]


def as_arrays(result, refs, queries, rows=None, sizes=None):
    """(off, recs as REC_FIELDS tuples, abund tuples, matched, n_cand, claimed, occ rows) over the selected rows, the others empty and zero"""
    plain = [(recs, matched, n_cand, claimed) for recs, _, matched, n_cand, claimed, _ in result]
    off, recs, matched, n_cand, claimed = sr.as_arrays(plain, refs, [list(m) for m in queries], rows, sizes)
    sel = set(range(len(queries)) if rows is None else rows)
    abund = [a for q, x in enumerate(result) if q in sel for a in x[1]]
    occ = [list(x[5]) if q in sel else [0, 0, 0] for q, x in enumerate(result)]
    return off, recs, abund, matched, n_cand, claimed, occ


def abund_tuples(abund):
    """a SCREEN_ABUND_DTYPE array as a list of ABUND_FIELDS tuples"""
    return [tuple(int(a[f]) for f in ABUND_FIELDS) for a in abund]


def holder_collections(n_ref, n_hash=5):
    """every collection of n_ref references and a query over n_hash hashes up to what cannot matter, as tests/test_screen_cpu.py argues: the
    query is the first k hashes, a collection the multiset of their holder sets times the number of hashes every reference holds outside the
    query.  Yields (refs, query hashes)."""
    for k in range(n_hash + 1):
        for holders in itertools.combinations_with_replacement(range(1 << n_ref), k):
            inside = [[h + 3 for h in range(k) if holders[h] >> r & 1] for r in range(n_ref)]
            for outside in itertools.product(range(n_hash - k + 1), repeat=n_ref):
                yield [inside[r] + [k + 3 + e for e in range(outside[r])] for r in range(n_ref)], [h + 3 for h in range(k)]


def small_collections(seed=3):
    """(refs, queries) for every collection of up to 3 references and 2 queries over 5 hashes in the sense of holder_collections -- the
    second query is every other hash of the first and one nobody indexes -- with counts from {1, 2, 3}: EVERY assignment of counts to the
    first query while it has at most 3 hashes and at most 2 references are there, two seeded draws otherwise; the second query's counts
    are drawn"""
    rng = np.random.default_rng(seed)
    for n_ref in (0, 1, 2, 3):
        for refs, query in holder_collections(n_ref):
            second = query[::2] + [99]
            if n_ref <= 2 and len(query) <= 3:
                draws = itertools.product((1, 2, 3), repeat=len(query))
            else:
                draws = [tuple(int(c) for c in rng.integers(1, 4, size=len(query))) for _ in range(2)]
            for counts in draws:
                yield refs, [dict(zip(query, counts)), {h: int(rng.integers(1, 4)) for h in second}]


# the edge list of tests/test_gpu_mask.py: the reference's `sub`, the intersection, and bands on either side of 1, 2 and 3 holders
MASK_BANDS = [(0, 0), (1, 0xFFFFFFFF), (0, 1), (2, 0xFFFFFFFF), (1, 2), (3, 3)]


def write_abund(path, sizes, counts):
    """a .sketch.abund side-car (rabbitkssd_amd/host/formats.hpp): the counts in the order the .sketch file stores its hashes"""
    with open(path, "wb") as f:
        f.write(b"RKABUND1" + struct.pack("<IIQ", len(sizes), 0, len(counts)) + np.asarray(sizes, dtype="<u4").tobytes() + np.asarray(counts, dtype="<u4").tobytes())


def with_counts(queries, rng, tail=True):
    """dicts hash -> count for hash arrays: geometric counts, most of them 1 to 10, with a tail"""
    out = []
    for q in queries:
        c = rng.geometric(0.35, size=len(q)).astype(np.int64)
        if tail and len(q):
            c[rng.random(len(q)) < 0.03] *= 1000
        out.append({int(h): int(x) for h, x in zip(q, c)})
    return out
